// SMJB blob -> DevModel.  Shared by the HIP library (uploads to device memory) and by the test-only lane
// emulator (host memory); `Up` supplies the two copy routines.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/smj.h"
#include "smj_model.h"

// The solver options that live in DevModel: (option name of smj_set_option or "" for none, field, type).  smj_set_solver_option sets a
// named one (smj_set_option on the primary model; the lane emulator), smj_step copies ALL of them onto the escalation model -- one list,
// so the two kernels, and the emulator that checks them, cannot run with different options.
// NOT here: row_limit ("primary_rows"): the escalation target keeps its full capacity.
#define SMJ_SOLVER_OPTIONS(X)                                                                                                             \
  X("iterations", iterations, int) X("tolerance", tolerance, float) X("warmstart", warmstart, int) X("pgs_fixed_iter", pgs_fixed_iter, int) \
  X("qcqp_exact", qcqp_exact, int) X("grad_noise", grad_noise, float) X("pgs_island_stop", pgs_island_stop, int)                            \
  X("max_contacts_per_pair", max_con_pair, int) X("solver", solver, int) X("convex_pairs", convex_pairs, int) X("multiccd", multiccd, int)  \
  X("sep_cache", sep_cache, int) X("manifold_cache", manifold_cache, int) X("pgs_dual_warmstart", pgs_dual_ws, int)                         \
  X("", ls_iterations, int) X("", multi_serial, int) X("", ls_tolerance, float)
static inline bool smj_set_solver_option(DevModel& m, const char* name, double v) {   // false: the list has no option of that name
#define X(opt, field, type) if ((opt)[0] && !strcmp(name, opt)) { m.field = (type)v; return true; }
  SMJ_SOLVER_OPTIONS(X)
#undef X
  return false;
}

// Binds a batch-major slot of DevState by its SMJ_SLOT_* number (include/smj.h).  false: not one of them -- SMJ_SLOT_CONTACTS is
// env-major with its own leading dimension, and is handed to the kernel only by a call that reads it (smj_step).
static inline bool smj_bind_slot(DevState& s, int slot, void* p) {
  switch (slot) {
    case SMJ_SLOT_QPOS: s.qpos = (float*)p; break;
    case SMJ_SLOT_QVEL: s.qvel = (float*)p; break;
    case SMJ_SLOT_CTRL: s.ctrl = (float*)p; break;
    case SMJ_SLOT_WARMSTART: s.warm = (float*)p; break;
    case SMJ_SLOT_NSTEP: s.nstep = (int*)p; break;
    case SMJ_SLOT_ACT_LENGTH: s.act_len = (float*)p; break;
    case SMJ_SLOT_ACT_VELOCITY: s.act_vel = (float*)p; break;
    case SMJ_SLOT_BASE_POSE: s.base = (float*)p; break;
    case SMJ_SLOT_GYRO: s.gyro = (float*)p; break;
    case SMJ_SLOT_ACCEL: s.accel = (float*)p; break;
    case SMJ_SLOT_LIDAR: s.lidar = (float*)p; break;
    case SMJ_SLOT_INFO: s.info = (int*)p; break;
    case SMJ_SLOT_DEBUG: s.debug = (float*)p; break;
    case SMJ_SLOT_PROF: s.prof = (float*)p; break;
    case SMJ_SLOT_XPOSE: s.xpose = (float*)p; break;
    case SMJ_SLOT_BASECTL: s.bctl = (float*)p; break;
    default: return false;
  }
  return true;
}

// Which of `caps` (the kernel variants available to the caller, smallest first) runs a model of m's dimensions: the first one it fits,
// -1 if none.  hint > 0 (k_capacity_hint of the model compiler, model_fuse.prepare_for_kernels: a contact-rich scene) skips the
// standard variant -- tall if the model fits it, else big -- and comes back to it last (a satellite model has its own builds).
static inline int smj_pick_variant(const DevModel& m, int hint, const SmjCaps* caps, int ncaps) {
  const int first = (hint > 0 && ncaps > 1) ? 1 : 0;
  for (int k = 0; k < ncaps; k++) {
    const SmjCaps& c = caps[(first + k) % ncaps];
    if ((m.nsat > 0) == (c.nsat > 0) && m.nsat <= c.nsat && m.nv <= (c.nvs ? c.nvs : c.nvp) && m.nbody <= c.nbp && m.nq <= c.nvp + 8 &&
        m.nldl <= c.nent * 64) return (first + k) % ncaps;
  }
  return -1;
}

struct SmjBlobEntry {
  char name[48];
  uint32_t dtype, ndim, shape[4];
  uint64_t offset, nbytes;
};

struct SmjBlob {
  const uint8_t* p;
  size_t n;
  // the entry table and every entry's payload lie inside the blob (a truncated / corrupt blob is rejected, not read past)
  bool valid() const {
    if (!p || n < 16) return false;
    uint32_t cnt;
    memcpy(&cnt, p + 8, 4);
    if ((size_t)cnt > (n - 16) / sizeof(SmjBlobEntry)) return false;
    const SmjBlobEntry* e = reinterpret_cast<const SmjBlobEntry*>(p + 16);
    for (uint32_t i = 0; i < cnt; i++)
      if (e[i].offset > n || e[i].nbytes > n - e[i].offset) return false;
    return true;
  }
  const SmjBlobEntry* find(const char* name) const {
    uint32_t cnt;
    memcpy(&cnt, p + 8, 4);
    const SmjBlobEntry* e = reinterpret_cast<const SmjBlobEntry*>(p + 16);
    for (uint32_t i = 0; i < cnt; i++)
      if (strncmp(e[i].name, name, 48) == 0) return &e[i];
    return nullptr;
  }
};

// The blob's tables on the host, by name, as the record builders read them: an index past a table's end reads 0.
struct SmjHostTables {
  std::map<std::string, std::vector<int>> i;
  std::map<std::string, std::vector<float>> f;
  int gi(const char* n, size_t k) { const std::vector<int>& v = i[n]; return k < v.size() ? v[k] : 0; }
  float gf(const char* n, size_t k) { const std::vector<float>& v = f[n]; return k < v.size() ? v[k] : 0.f; }
  static int fb(float v) { int b; memcpy(&b, &v, 4); return b; }   // a float's bit pattern: how the records hold floats
};

// Host restatement of what the kernel's stage-table loaders (smj_step_impl.h: KinTab, BodyTab, DofTab, EntryTab, ActTab)
// used to gather per lane from the individual tables, one record per lane; the positions are the SMJ_KIN_* .. SMJ_ACT_* of smj_model.h.
// nent: capacity of a kernel variant (smj_model.h) -- the loader builds its records for the variant that will run
static inline std::vector<int> smj_build_lanerec(const DevModel& m, SmjHostTables& T, int nent) {
  const int LR_ACT = smj_lr_act(nent), LR_STRIDE = smj_lr_stride(nent);
  std::vector<int> rec(64 * LR_STRIDE, 0);
  const int nb = m.nbody, nv = m.nv, nu = m.nu;
  for (int L = 0; L < 64; L++) {
    int* r = rec.data() + L * LR_STRIDE;
    {  // KinTab: parent, level, jump[6], pos[3], quat[4], jtype[2], jqadr[2], jdadr[2], jq0[2], jaxis[6], jpos[6]
      int* k = r + SMJ_LR_KIN;
      const int b = L < nb ? L : 0;
      k[SMJ_KIN_PARENT] = T.gi("body_parentid", b); k[SMJ_KIN_LEVEL] = L < nb ? T.gi("k_body_level", b) : -1;
      for (int q = 0; q < 6; q++) k[SMJ_KIN_JUMP + q] = (q < m.njump && L > 0 && L < nb) ? T.gi("k_body_jump", q * nb + b) : 0;
      for (int q = 0; q < 3; q++) k[SMJ_KIN_POS + q] = T.fb(T.gf("body_pos", 3 * b + q));
      for (int q = 0; q < 4; q++) k[SMJ_KIN_QUAT + q] = T.fb(T.gf("body_quat", 4 * b + q));
      const int jn = T.gi("body_jntnum", b), ja = T.gi("body_jntadr", b);
      for (int u = 0; u < 2; u++) {
        const int jj = (L < nb && u < jn) ? ja + u : -1, jx = jj >= 0 ? jj : 0, qa = T.gi("jnt_qposadr", jx);
        k[SMJ_KIN_JTYPE + u] = jj >= 0 ? T.gi("jnt_type", jx) : -1; k[SMJ_KIN_JQADR + u] = qa; k[SMJ_KIN_JDADR + u] = T.gi("jnt_dofadr", jx); k[SMJ_KIN_JQ0 + u] = T.fb(T.gf("qpos0", qa));
        for (int q = 0; q < 3; q++) { k[SMJ_KIN_JAXIS + 3 * u + q] = T.fb(T.gf("jnt_axis", 3 * jx + q)); k[SMJ_KIN_JPOS + 3 * u + q] = T.fb(T.gf("jnt_pos", 3 * jx + q)); }
      }
    }
    {  // BodyTab: root, subsize, parent, dofadr, dofnum, jump[6], dofmask lo, hi, inertia_local[10]
      int* k = r + SMJ_LR_BODY;
      const int b = L < nb ? L : 0;
      k[SMJ_BODY_ROOT] = T.gi("body_rootid", b); k[SMJ_BODY_SUBSIZE] = T.gi("k_body_subtreesize", b); k[SMJ_BODY_PARENT] = T.gi("body_parentid", b);
      k[SMJ_BODY_DOFADR] = T.gi("body_dofadr", b); k[SMJ_BODY_DOFNUM] = L < nb ? T.gi("body_dofnum", b) : 0;
      for (int q = 0; q < 6; q++) k[SMJ_BODY_JUMP + q] = (q < m.njump && L > 0 && L < nb) ? T.gi("k_body_jump", q * nb + b) : 0;
      k[SMJ_BODY_DOFMASK_LO] = T.gi("k_body_dofmask_lo", b); k[SMJ_BODY_DOFMASK_HI] = T.gi("k_body_dofmask_hi", b);
      for (int q = 0; q < 10; q++) k[SMJ_BODY_INL + q] = T.fb(T.gf("k_body_inertia_local", 10 * b + q));
    }
    {  // DofTab: body, jtype, qadr, first, bsub, velmask lo, hi, damp, stiff, spring, act[2], actmom[2]
      int* k = r + SMJ_LR_DOF;
      const int d = L < nv ? L : 0, j = T.gi("dof_jntid", d), db = T.gi("dof_bodyid", d), jt = T.gi("jnt_type", j);
      k[SMJ_DOF_BODY] = db; k[SMJ_DOF_JTYPE] = jt; k[SMJ_DOF_QADR] = T.gi("k_dof_qposadr", d); k[SMJ_DOF_FIRST] = T.gi("jnt_dofadr", j);
      k[SMJ_DOF_BSUB] = T.gi("k_body_subtreesize", db); k[SMJ_DOF_VELMASK_LO] = T.gi("k_dof_velmask_lo", d); k[SMJ_DOF_VELMASK_HI] = T.gi("k_dof_velmask_hi", d);
      k[SMJ_DOF_DAMP] = T.fb(T.gf("dof_damping", d));
      k[SMJ_DOF_STIFF] = T.fb(jt == 0 ? 0.f : T.gf("jnt_stiffness", j));
      k[SMJ_DOF_SPRING] = T.fb(jt == 0 ? 0.f : T.gf("qpos_spring", T.gi("jnt_qposadr", j)));
      for (int u = 0; u < 2; u++) { k[SMJ_DOF_ACT + u] = T.gi("k_dof_act", 2 * d + u); k[SMJ_DOF_ACTMOM + u] = T.fb(T.gf("k_dof_actmom", 2 * d + u)); }
    }
    {  // EntryTab, `nent` mass-matrix pattern slots: i[], j[], arm[] | lact[], damp[], dcoef[], lcoef[] (implicit only)
      int* k = r + SMJ_LR_ENT;
      for (int u = 0; u < nent; u++) {
        const int e = L + 64 * u, ok = e < m.nldl, ex = ok ? e : 0, i = T.gi("k_ldl_i", ex), j = T.gi("k_ldl_j", ex);
        k[SMJ_ENT_I * nent + u] = ok ? i : -1; k[SMJ_ENT_J * nent + u] = ok ? j : 0; k[SMJ_ENT_ARM * nent + u] = T.fb((ok && i == j) ? T.gf("dof_armature", i) : 0.f);
        k[SMJ_ENT_LACT * nent + u] = ok ? T.gi("k_ldl_lact", ex) : -1;
        k[SMJ_ENT_DAMP * nent + u] = T.fb(ok ? T.gf("k_ldl_damp", ex) : 0.f); k[SMJ_ENT_DCOEF * nent + u] = T.fb(ok ? T.gf("k_ldl_dcoef", ex) : 0.f); k[SMJ_ENT_LCOEF * nent + u] = T.fb(ok ? T.gf("k_ldl_lcoef", ex) : 0.f);
      }
    }
    {  // ActTab: dof[4], qadr[4], mom[4], prm[8], flags, gc_body, gc_mlo, gc_mhi, gc_mass, gc_x, gc_y, gc_z
      int* k = r + LR_ACT;
      const int a = L < nu ? L : 0;
      for (int u = 0; u < 4; u++) {
        const int dd = T.gi("k_act_dof", 4 * a + u);
        k[SMJ_ACT_DOF + u] = L < nu ? dd : -1; k[SMJ_ACT_QADR + u] = dd >= 0 ? T.gi("k_dof_qposadr", dd) : 0; k[SMJ_ACT_MOM + u] = T.fb(T.gf("k_act_mom", 4 * a + u));
      }
      k[SMJ_ACT_GAIN] = T.fb(T.gf("actuator_gainprm", 3 * a));
      for (int q = 0; q < 3; q++) k[SMJ_ACT_BIAS + q] = T.fb(T.gf("actuator_biasprm", 3 * a + q));
      for (int q = 0; q < 2; q++) { k[SMJ_ACT_CTRLRANGE + q] = T.fb(T.gf("actuator_ctrlrange", 2 * a + q)); k[SMJ_ACT_FORCERANGE + q] = T.fb(T.gf("actuator_forcerange", 2 * a + q)); }
      k[SMJ_ACT_FLAGS] = (T.gi("actuator_ctrllimited", a) ? 1 : 0) | (T.gi("actuator_forcelimited", a) ? 2 : 0) | (T.gi("actuator_biastype", a) == 1 ? 4 : 0);
      const int g = L < m.ngc ? T.gi("k_gc_body", L) : 0;
      k[SMJ_ACT_GC_BODY] = g; k[SMJ_ACT_GC_MLO] = T.gi("k_body_dofmask_lo", g); k[SMJ_ACT_GC_MHI] = T.gi("k_body_dofmask_hi", g);
      k[SMJ_ACT_GC_MASS] = T.fb(L < m.ngc ? T.gf("body_gcmass", g) : 0.f);
      for (int q = 0; q < 3; q++) k[SMJ_ACT_GC_POS + q] = T.fb(T.gf("body_gcipos", 3 * g + q));
    }
  }
  return rec;
}

static inline std::vector<int> smj_build_pprec(const DevModel& m, SmjHostTables& T) {
  std::vector<int> rec((size_t)(m.nplanepair > 0 ? m.nplanepair : 1) * SMJ_PP_STRIDE, 0);
  for (int t = 0; t < m.nplanepair; t++) {
    int* k = rec.data() + (size_t)t * SMJ_PP_STRIDE;
    const int p = T.gi("k_planepair", t), g1 = T.gi("pair_geom1", p), g2 = T.gi("pair_geom2", p);
    k[SMJ_PP_PAIR] = p; k[SMJ_PP_G1] = g1; k[SMJ_PP_G2] = g2; k[SMJ_PP_B1] = T.gi("geom_bodyid", g1); k[SMJ_PP_B2] = T.gi("geom_bodyid", g2);
    k[SMJ_PP_T2] = T.gi("geom_type", g2); k[SMJ_PP_MARGIN] = T.fb(T.gf("pair_margin", p)); k[SMJ_PP_RBOUND2] = T.fb(T.gf("geom_rbound", g2));
    for (int q = 0; q < 3; q++) {
      k[SMJ_PP_BCEN2 + q] = T.fb(T.gf("k_geom_bcenter", 3 * g2 + q));
      k[SMJ_PP_POS1 + q] = T.fb(T.gf("geom_pos", 3 * g1 + q)); k[SMJ_PP_POS2 + q] = T.fb(T.gf("geom_pos", 3 * g2 + q));
      k[SMJ_PP_SIZE2 + q] = T.fb(T.gf("geom_size", 3 * g2 + q));
    }
    for (int q = 0; q < 9; q++) { k[SMJ_PP_MAT1 + q] = T.fb(T.gf("k_geom_mat", 9 * g1 + q)); k[SMJ_PP_MAT2 + q] = T.fb(T.gf("k_geom_mat", 9 * g2 + q)); }
    k[SMJ_PP_CONDIM] = T.gi("pair_condim", p); k[SMJ_PP_MG] = T.fb(T.gf("pair_margin", p) - T.gf("pair_gap", p));
    for (int q = 0; q < 5; q++) { k[SMJ_PP_FRIC + q] = T.fb(T.gf("pair_friction", 5 * p + q)); k[SMJ_PP_SOLIMP + q] = T.fb(T.gf("pair_solimp", 5 * p + q)); }
    k[SMJ_PP_SOLREF] = T.fb(T.gf("pair_solref", 2 * p)); k[SMJ_PP_SOLREF + 1] = T.fb(T.gf("pair_solref", 2 * p + 1));
    for (int q = 0; q < 6; q++) k[SMJ_PP_BOX2 + q] = T.fb(T.gf("geom_aabb", 6 * g2 + q));
  }
  return rec;
}
static inline std::vector<int> smj_build_cgrec(const DevModel& m, SmjHostTables& T, bool stat = false) {
  const int ncg = stat ? m.nsgeom : m.ncgeom;
  std::vector<int> rec((size_t)(ncg > 0 ? ncg : 1) * SMJ_CG_STRIDE, 0);
  for (int c = 0; c < ncg; c++) {
    int* k = rec.data() + (size_t)c * SMJ_CG_STRIDE;
    const int g = T.gi(stat ? "k_sgeom" : "k_cgeom", c), adr = T.gi("geom_hulladr", g);
    k[SMJ_CG_GEOM] = g; k[SMJ_CG_BODY] = T.gi("geom_bodyid", g);
    k[SMJ_CG_META] = (int)((unsigned)T.gi("geom_type", g) | ((unsigned)T.gi("geom_hullnum", g) << 4) | ((unsigned)(adr < 0 ? 0 : adr) << 16));
    for (int q = 0; q < 3; q++) {
      k[SMJ_CG_POS + q] = T.fb(T.gf("geom_pos", 3 * g + q)); k[SMJ_CG_LCEN + q] = T.fb(T.gf("geom_aabb", 6 * g + q));
      k[SMJ_CG_HALF + q] = T.fb(T.gf("geom_aabb", 6 * g + 3 + q)); k[SMJ_CG_CCEN + q] = T.fb(T.gf("geom_ccenter", 3 * g + q));
      k[SMJ_CG_SIZE + q] = T.fb(T.gf("geom_size", 3 * g + q));
    }
    for (int q = 0; q < 9; q++) k[SMJ_CG_MAT + q] = T.fb(T.gf("k_geom_mat", 9 * g + q));
    k[SMJ_CG_RBOUND] = T.fb(T.gf("geom_rbound", g));
  }
  return rec;
}

static inline std::vector<int> smj_build_rowrec(const DevModel& m, SmjHostTables& T) {
  const int nstat = m.neq + m.nfric, n = nstat + 2 * m.nlimit;
  std::vector<int> rec((size_t)(n > 0 ? n : 1) * SMJ_RR_STRIDE, 0);
  for (int e = 0; e < m.neq; e++) {      // CT_EQUALITY = 0 (joint equalities)
    int* k = rec.data() + (size_t)e * SMJ_RR_STRIDE;
    const int j1 = T.gi("eq_obj1id", e), j2 = T.gi("eq_obj2id", e), q1 = T.gi("jnt_qposadr", j1), d1 = T.gi("jnt_dofadr", j1);
    k[SMJ_RR_TYPE] = 0; k[SMJ_RR_ID] = e; k[SMJ_RR_SAT] = -1; k[SMJ_RR_D1] = d1; k[SMJ_RR_Q1] = q1; k[SMJ_RR_V1] = T.fb(T.gf("qpos0", q1));
    float diag = T.gf("dof_invweight0", d1);
    if (j2 >= 0) {
      const int q2 = T.gi("jnt_qposadr", j2), d2 = T.gi("jnt_dofadr", j2);
      k[SMJ_RR_D2] = d2; k[SMJ_RR_Q2] = q2; k[SMJ_RR_V2] = T.fb(T.gf("qpos0", q2));
      diag += T.gf("dof_invweight0", d2);
    } else { k[SMJ_RR_D2] = -1; k[SMJ_RR_Q2] = 0; }
    for (int q = 0; q < 5; q++) { k[SMJ_RR_DATA + q] = T.fb(T.gf("eq_data", 5 * e + q)); k[SMJ_RR_SOLIMP + q] = T.fb(T.gf("eq_solimp", 5 * e + q)); }
    k[SMJ_RR_DIAG] = T.fb(diag);
    k[SMJ_RR_SOLREF] = T.fb(T.gf("eq_solref", 2 * e)); k[SMJ_RR_SOLREF + 1] = T.fb(T.gf("eq_solref", 2 * e + 1));
  }
  // (satellite of a dof / its index inside it; -1, 0 for dofs of the main tree)
  auto sat_of = [&](int d, int* local) {
    *local = 0;
    for (int sidx = 0; sidx < m.nsat; sidx++) {
      const int da = T.gi("k_sat_i", SMJ_SAT_I_STRIDE * sidx + SMJ_SR_DADR), nd = T.gi("k_sat_i", SMJ_SAT_I_STRIDE * sidx + SMJ_SR_NDOF);
      if (d >= da && d < da + nd) { *local = d - da; return sidx; }
    }
    return -1;
  };
  for (int f = 0; f < m.nfric; f++) {    // CT_FRICTION = 1
    int* k = rec.data() + (size_t)(m.neq + f) * SMJ_RR_STRIDE;
    const int d = T.gi("k_fric_dof", f);
    k[SMJ_RR_SAT] = sat_of(d, &k[SMJ_RR_SDOF]);
    k[SMJ_RR_TYPE] = 1; k[SMJ_RR_ID] = d; k[SMJ_RR_D1] = d; k[SMJ_RR_D2] = -1;
    k[SMJ_RR_DIAG] = T.fb(T.gf("dof_invweight0", d)); k[SMJ_RR_FLOSS] = T.fb(T.gf("dof_frictionloss", d));
    k[SMJ_RR_SOLREF] = T.fb(T.gf("dof_solref", 2 * d)); k[SMJ_RR_SOLREF + 1] = T.fb(T.gf("dof_solref", 2 * d + 1));
    for (int q = 0; q < 5; q++) k[SMJ_RR_SOLIMP + q] = T.fb(T.gf("dof_solimp", 5 * d + q));
  }
  for (int L = 0; L < 2 * m.nlimit; L++) {   // CT_LIMIT = 3; slot L = (joint, side), lower side first
    int* k = rec.data() + (size_t)(nstat + L) * SMJ_RR_STRIDE;
    const int j = T.gi("k_limit_jnt", L >> 1), d = T.gi("jnt_dofadr", j);
    k[SMJ_RR_SAT] = sat_of(d, &k[SMJ_RR_SDOF]);
    k[SMJ_RR_TYPE] = 3; k[SMJ_RR_ID] = j; k[SMJ_RR_D1] = d; k[SMJ_RR_D2] = (L & 1) ? 1 : -1; k[SMJ_RR_Q1] = T.gi("jnt_qposadr", j);
    k[SMJ_RR_V1] = T.fb(T.gf("jnt_range", 2 * j + (L & 1))); k[SMJ_RR_V2] = T.fb(T.gf("jnt_margin", j));
    k[SMJ_RR_DIAG] = T.fb(T.gf("dof_invweight0", d));
    k[SMJ_RR_SOLREF] = T.fb(T.gf("jnt_solref", 2 * j)); k[SMJ_RR_SOLREF + 1] = T.fb(T.gf("jnt_solref", 2 * j + 1));
    for (int q = 0; q < 5; q++) k[SMJ_RR_SOLIMP + q] = T.fb(T.gf("jnt_solimp", 5 * j + q));
  }
  return rec;
}

static inline std::vector<int> smj_build_cprec(const DevModel& m, SmjHostTables& T, bool stat = false) {
  const int np = stat ? m.nstatpair : m.nconvpair;
  std::vector<int> rec((size_t)(np > 0 ? np : 1) * SMJ_CP_STRIDE, 0);
  std::map<int, int> dslot, sslot;   // static pairs: geom -> cache slot of the moving geom / index of the static geom
  if (stat) {
    for (int c = 0; c < m.ncgeom; c++) dslot[T.gi("k_cgeom", c)] = c;
    for (int c = 0; c < m.nsgeom; c++) sslot[T.gi("k_sgeom", c)] = c;
  }
  for (int t = 0; t < np; t++) {
    int* k = rec.data() + (size_t)t * SMJ_CP_STRIDE;
    const int p = T.gi(stat ? "k_statpair" : "k_convpair", t);
    k[SMJ_CP_PAIR] = p; k[SMJ_CP_G1] = T.gi("pair_geom1", p); k[SMJ_CP_G2] = T.gi("pair_geom2", p);
    if (stat) {
      k[SMJ_CP_S1] = sslot.count(k[SMJ_CP_G1]) ? -1 - sslot[k[SMJ_CP_G1]] : dslot[k[SMJ_CP_G1]];
      k[SMJ_CP_S2] = sslot.count(k[SMJ_CP_G2]) ? -1 - sslot[k[SMJ_CP_G2]] : dslot[k[SMJ_CP_G2]];
    } else { k[SMJ_CP_S1] = T.gi("k_convpair_s1", t); k[SMJ_CP_S2] = T.gi("k_convpair_s2", t); }
    k[SMJ_CP_MARGIN] = T.fb(T.gf("pair_margin", p)); k[SMJ_CP_MG] = T.fb(T.gf("pair_margin", p) - T.gf("pair_gap", p)); k[SMJ_CP_CONDIM] = T.gi("pair_condim", p);
    for (int q = 0; q < 5; q++) { k[SMJ_CP_FRIC + q] = T.fb(T.gf("pair_friction", 5 * p + q)); k[SMJ_CP_SOLIMP + q] = T.fb(T.gf("pair_solimp", 5 * p + q)); }
    k[SMJ_CP_SOLREF] = T.fb(T.gf("pair_solref", 2 * p)); k[SMJ_CP_SOLREF + 1] = T.fb(T.gf("pair_solref", 2 * p + 1));
    const float r1 = T.gf("geom_rbound", k[SMJ_CP_G1]), r2 = T.gf("geom_rbound", k[SMJ_CP_G2]);
    k[SMJ_CP_RBMIN] = T.fb(r1 < r2 ? r1 : r2);
    k[SMJ_CP_B1] = T.gi("geom_bodyid", k[SMJ_CP_G1]); k[SMJ_CP_B2] = T.gi("geom_bodyid", k[SMJ_CP_G2]);
  }
  return rec;
}

// One table of the blob as host words: an i32 entry as it stands, an f64 entry rounded to fp32; never empty (a table without elements
// is one zero word).  false: the blob has no entry of that name and type.
static inline bool smj_read_i32(const SmjBlob& b, const char* name, std::vector<int>& h) {
  const SmjBlobEntry* e = b.find(name);
  if (!e || e->dtype != 1) return false;
  h.assign(e->nbytes / 4 ? e->nbytes / 4 : 1, 0);
  memcpy(h.data(), b.p + e->offset, e->nbytes / 4 * 4);
  return true;
}
static inline bool smj_read_f64(const SmjBlob& b, const char* name, std::vector<float>& h) {
  const SmjBlobEntry* e = b.find(name);
  if (!e || e->dtype != 0) return false;
  const size_t cnt = e->nbytes / 8;
  h.assign(cnt ? cnt : 1, 0.f);
  const double* src = reinterpret_cast<const double*>(b.p + e->offset);
  for (size_t i = 0; i < cnt; i++) h[i] = (float)src[i];
  return true;
}

// Defaults of the solver options (SMJ_SOLVER_OPTIONS) and of the two per-launch fields; after the model's dimensions are known.
static inline void smj_solver_defaults(DevModel& m) {
  m.row_limit = 0;
  m.pgs_cap = 0;
  m.warmstart = 1;
  m.pgs_fixed_iter = 0;
  m.qcqp_exact = 0;
  m.grad_noise = 4e-6f;
  m.pgs_island_stop = 1;
  m.pgs_dual_ws = 1;
  m.max_con_pair = 4;
  m.solver = 0;
  m.convex_pairs = 1;
  m.multiccd = 1;
  m.sep_cache = getenv("SMJ_NO_SEPCACHE") ? 0 : 1;
  // pays where free objects rest; a robot alone (<= 32 dofs) has no resting convex pair and the lookup cost the headline 1 %
  m.manifold_cache = (getenv("SMJ_NO_MCACHE") || m.nv_all <= 32) ? 0 : 1;
  m.multi_serial = 0;
  m.ls_iterations = 50;
  m.ls_tolerance = 0.01f;
}

// `caps`: the kernel variants available to the caller, smallest first; the first one the model fits is chosen (*chosen).
template <class Up>
int smj_load_model(const void* blob, size_t nbytes, DevModel& m, Up& up, std::string& err, const SmjCaps* caps, int ncaps, int* chosen) {
  if (!blob || nbytes < 16 || memcmp(blob, "SMJB0001", 8) != 0) { err = "not an SMJB model blob"; return -1; }
  SmjBlob b{static_cast<const uint8_t*>(blob), nbytes};
  if (!b.valid()) { err = "model blob: truncated or corrupt entry table"; return -3; }
  auto geti = [&](const char* name, int idx, int* out) -> bool {
    const SmjBlobEntry* e = b.find(name);
    if (!e || e->dtype != 1 || e->nbytes < 4u * (idx + 1)) { err = std::string("model blob: missing int ") + name; return false; }
    memcpy(out, b.p + e->offset + 4 * idx, 4);
    return true;
  };
  auto getf = [&](const char* name, int idx, float* out) -> bool {
    const SmjBlobEntry* e = b.find(name);
    if (!e || e->dtype != 0 || e->nbytes < 8u * (idx + 1)) { err = std::string("model blob: missing scalar ") + name; return false; }
    double v;
    memcpy(&v, b.p + e->offset + 8 * idx, 8);
    *out = (float)v;
    return true;
  };
#define GI(field, name, idx) if (!geti(name, idx, &m.field)) return -3;
#define GF(field, name, idx) if (!getf(name, idx, &m.field)) return -3;
  GI(nq_all, "dims", 0) GI(nv_all, "dims", 1) GI(nu, "dims", 2) GI(nbody_all, "dims", 3) GI(njnt, "dims", 4) GI(ngeom, "dims", 5)
  m.nq = m.nq_all; m.nv = m.nv_all; m.nbody = m.nbody_all; m.nsat = 0;
  if (b.find("k_nsat")) {   // satellites (model_fuse.find_satellites): the main part's counts index the lane tables
    GI(nsat, "k_nsat", 0)
    if (m.nsat > 0) { GI(nq, "k_main_dims", 0) GI(nv, "k_main_dims", 1) GI(nbody, "k_main_dims", 2) GI(njnt, "k_main_dims", 3) }
  }
  GI(nsite, "dims", 6) GI(neq, "dims", 8) GI(nkey, "dims", 11) GI(npair, "dims", 12)
  GI(nlevel, "k_nlevel", 0) GI(nfric, "k_nfric", 0) GI(nlimit, "k_nlimit", 0) GI(nplanepair, "k_nplanepair", 0)
  GI(nldl, "k_nldl", 0) GI(imu_site, "sensor_imu_site", 0) GI(ngc, "k_ngc", 0) GI(nroot, "k_nroot", 0)
  GI(njump, "k_njump", 0) GI(maxsubtree, "k_maxsubtree", 0) GI(ncgeom, "k_ncgeom", 0) GI(nconvpair, "k_nconvpair", 0) GI(iterations, "opt_iterations", 0)
  GF(timestep, "opt_timestep", 0) GF(gravity[0], "opt_gravity", 0) GF(gravity[1], "opt_gravity", 1)
  GF(gravity[2], "opt_gravity", 2) GF(impratio, "opt_impratio", 0) GF(tolerance, "opt_tolerance", 0)
  GF(meaninertia, "stat_meaninertia", 0) GF(lidar_cutoff, "sensor_lidar_cutoff", 0)
#undef GI
#undef GF
  if (m.nsat > 0 && (m.ngeom >= 65536 || m.npair >= (1 << 19))) { err = "satellite builds: at most 65535 geoms and 524287 collision pairs (16-bit geom ids per contact, the PGS row key)"; return -4; }
  const SmjBlobEntry* lidar = b.find("sensor_lidar_site");
  m.nlidar = lidar ? (int)(lidar->nbytes / 4) : 0;
  smj_solver_defaults(m);
  char buf[256];
  std::vector<int> hint(1, 0);   // optional hint of the model compiler: contact-rich scene (smj_pick_variant)
  smj_read_i32(b, "k_capacity_hint", hint);
  const int pick = smj_pick_variant(m, hint[0], caps, ncaps);
  if (pick < 0 || m.nu > 16) {
    const SmjCaps& c = caps[ncaps - 1];
    snprintf(buf, sizeof buf, "model exceeds kernel capacity (nv %d<=%d, nbody %d<=%d, nq %d<=%d, nu %d<=16, mass-matrix entries %d<=%d, satellites %d)",
             m.nv, c.nvp, m.nbody, c.nbp, m.nq, c.nvp + 8, m.nu, m.nldl, c.nent * 64, m.nsat);
    err = buf;
    return -4;
  }
  if (chosen) *chosen = pick;
  const int nent = caps[pick].nent;
  if (m.neq + m.nfric > 64) { err = "too many static constraint rows"; return -4; }
  if (2 * m.nlimit > 64) { err = "too many limited joints"; return -4; }
  if (m.ngc > 16) { err = "more than 16 gravity-compensated bodies"; return -4; }
  if (m.njump > 6) { err = "body tree deeper than 64 levels"; return -4; }
  if (m.ncgeom > NCG) { err = "too many geoms in non-plane collision pairs"; return -4; }
  if (m.nconvpair >= 65536) { err = "more than 65535 non-plane collision pairs (the survivor list holds 16-bit pair indices)"; return -4; }
  SmjHostTables T;
#define X(n)                                                                                     \
  if (!smj_read_i32(b, #n, T.i[#n])) { err = "model blob: missing i32 array " #n; return -3; }   \
  if (!(m.n = up.i32(T.i[#n]))) { err = "device allocation failed for " #n; return -2; }
  SMJ_MODEL_I32(X)
#undef X
#define X(n)                                                                                     \
  if (!smj_read_f64(b, #n, T.f[#n])) { err = "model blob: missing f64 array " #n; return -3; }   \
  if (!(m.n = up.f32(T.f[#n]))) { err = "device allocation failed for " #n; return -2; }
  SMJ_MODEL_F32(X)
#undef X
  m.nsgeom = 0; m.nstatpair = 0; m.k_sgrec = m.k_sprec = m.k_spair = m.k_grid_adr = m.k_grid_list = m.k_sg_cell = nullptr; m.k_sg_bound = nullptr; m.k_sgw = nullptr;
  if (b.find("k_nsgeom")) {
    if (!geti("k_nsgeom", 0, &m.nsgeom) || !geti("k_nstatpair", 0, &m.nstatpair)) return -3;
    if (m.nsgeom > 512) { err = "more than 512 static collision geoms (the static broadphase's candidate word holds 9 bits of static geom index)"; return -4; }
    if (m.nstatpair > 0 && m.nsat == 0) { err = "static collision pairs (k_statpair) without satellites: only the satellite builds run collision_static; rebuild the blob (model_fuse.prepare_for_kernels)"; return -4; }
    if (m.nsgeom > 0) {
      for (int q = 0; q < 3; q++) { if (!geti("k_grid", q, &m.grid_dim[q]) || !getf("k_grid_f", q, &m.grid_org[q])) return -3; }
      if (!getf("k_grid_f", 3, &m.grid_h) || !getf("k_grid_f", 4, &m.grid_margin)) return -3;
      auto loadi = [&](const char* name) -> const int* {   // (k_sgeom, k_statpair: read by the record builders only)
        if (!smj_read_i32(b, name, T.i[name])) { err = std::string("model blob: missing i32 array ") + name; return nullptr; }
        return up.i32(T.i[name]);
      };
      if (!loadi("k_sgeom") || !loadi("k_statpair") || !(m.k_spair = loadi("k_spair")) || !(m.k_grid_adr = loadi("k_grid_adr")) ||
          !(m.k_grid_list = loadi("k_grid_list")) || !(m.k_sg_cell = loadi("k_sg_cell"))) return err.empty() ? -2 : -3;
      std::vector<int> sg = smj_build_cgrec(m, T, true), spr = smj_build_cprec(m, T, true);
      m.k_sgrec = up.i32(sg);
      m.k_sprec = up.i32(spr);
      // each static geom in the world frame (SMJ_SGW_*) and the world AABB of its oriented box (SMJ_SGB_*: lo xyz, pad, hi xyz, pad)
      std::vector<float> bound(SMJ_SGB_STRIDE * (size_t)m.nsgeom, 0.f), sgw(SMJ_SGW_STRIDE * (size_t)m.nsgeom, 0.f);
      for (int c = 0; c < m.nsgeom; c++) {
        const int* k = sg.data() + (size_t)c * SMJ_CG_STRIDE;
        float f[SMJ_CG_STRIDE];
        memcpy(f, k, sizeof f);
        float *w = sgw.data() + SMJ_SGW_STRIDE * (size_t)c, *bd = bound.data() + SMJ_SGB_STRIDE * (size_t)c;
        for (int i = 0; i < 3; i++) {
          const float cen = f[SMJ_CG_POS + i] + f[SMJ_CG_MAT + 3 * i] * f[SMJ_CG_LCEN] + f[SMJ_CG_MAT + 3 * i + 1] * f[SMJ_CG_LCEN + 1] + f[SMJ_CG_MAT + 3 * i + 2] * f[SMJ_CG_LCEN + 2];
          const float ext = fabsf(f[SMJ_CG_MAT + 3 * i]) * f[SMJ_CG_HALF] + fabsf(f[SMJ_CG_MAT + 3 * i + 1]) * f[SMJ_CG_HALF + 1] + fabsf(f[SMJ_CG_MAT + 3 * i + 2]) * f[SMJ_CG_HALF + 2];
          bd[SMJ_SGB_LO + i] = cen - ext; bd[SMJ_SGB_HI + i] = cen + ext;
          w[SMJ_SGW_POS + i] = f[SMJ_CG_POS + i]; w[SMJ_SGW_CEN + i] = cen; w[SMJ_SGW_HALF + i] = f[SMJ_CG_HALF + i]; w[SMJ_SGW_SIZE + i] = f[SMJ_CG_SIZE + i];
          w[SMJ_SGW_CCEN + i] = f[SMJ_CG_POS + i] + f[SMJ_CG_MAT + 3 * i] * f[SMJ_CG_CCEN] + f[SMJ_CG_MAT + 3 * i + 1] * f[SMJ_CG_CCEN + 1] + f[SMJ_CG_MAT + 3 * i + 2] * f[SMJ_CG_CCEN + 2];
        }
        for (int i = 0; i < 9; i++) w[SMJ_SGW_MAT + i] = f[SMJ_CG_MAT + i];
        memcpy(&w[SMJ_SGW_META], &k[SMJ_CG_META], 4);
      }
      m.k_sg_bound = up.f32(bound);
      m.k_sgw = up.f32(sgw);
      if (!m.k_sgrec || !m.k_sprec || !m.k_sg_bound || !m.k_sgw) { err = "device allocation failed for the static-geometry tables"; return -2; }
    }
  }
  m.nfric_main = m.nfric; m.nlimit_main = m.nlimit; m.k_satrec = nullptr;
  if (m.nsat > 0) {
    std::vector<int>& si = T.i["k_sat_i"];
    std::vector<float> sf;
    if (!smj_read_i32(b, "k_sat_i", si) || !smj_read_f64(b, "k_sat_f", sf) || si.size() < SMJ_SAT_I_STRIDE * (size_t)m.nsat || sf.size() < SMJ_SAT_F_STRIDE * (size_t)m.nsat) { err = "model blob: satellite tables missing"; return -3; }
    std::vector<int> rec((size_t)m.nsat * SMJ_SR_STRIDE, 0);
    for (int sidx = 0; sidx < m.nsat; sidx++) {
      int* k = rec.data() + (size_t)sidx * SMJ_SR_STRIDE;
      for (int q = 0; q < SMJ_SAT_I_STRIDE; q++) k[q] = si[SMJ_SAT_I_STRIDE * sidx + q];
      for (int q = 0; q < SMJ_SAT_F_STRIDE; q++) k[SMJ_SR_F + q] = T.fb(sf[SMJ_SAT_F_STRIDE * sidx + q]);
    }
    m.k_satrec = up.i32(rec);
    if (!m.k_satrec) { err = "device allocation failed for k_satrec"; return -2; }
    // static rows / limit slots of the main tree come first in their tables (dof / joint order)
    m.nfric_main = m.nlimit_main = 0;
    for (int f = 0; f < m.nfric; f++) m.nfric_main += T.i["k_fric_dof"][f] < m.nv;
    for (int L = 0; L < m.nlimit; L++) m.nlimit_main += T.i["jnt_dofadr"][T.i["k_limit_jnt"][L]] < m.nv;
  }
  m.k_lanerec = up.i32(smj_build_lanerec(m, T, nent));
  if (!m.k_lanerec) { err = "device allocation failed for k_lanerec"; return -2; }
  m.k_pprec = up.i32(smj_build_pprec(m, T));
  m.k_cgrec = up.i32(smj_build_cgrec(m, T));
  if (!m.k_pprec || !m.k_cgrec) { err = "device allocation failed for the collision records"; return -2; }
  m.k_rowrec = up.i32(smj_build_rowrec(m, T));
  if (!m.k_rowrec) { err = "device allocation failed for k_rowrec"; return -2; }
  m.k_cprec = up.i32(smj_build_cprec(m, T));
  if (!m.k_cprec) { err = "device allocation failed for k_cprec"; return -2; }
  return 0;
}
