// TEST INFRASTRUCTURE ONLY -- lane emulator of the HIP step kernel.
//
// Compiles stretch_mujoco_amd/csrc/smj_step_impl.h with SMJ_EMUL (smj_wave.h): every lane region becomes a
// loop over 64 lanes and cross-lane ops act on arrays, in fp32, with the same operation order as the GPU
// code.  It exists so that the kernel LOGIC can be checked against the fp64 oracle on a machine without a
// GPU (`pytest -m "not gpu"`).  It is never linked into libsmj.so and nothing in stretch_mujoco_amd/ loads it.
//
// One library per build of the table in csrc/smj_builds.h: libsmj_emul_<tag>.so is this file with -DSMJ_BUILD_TAG=<tag> (Makefile) and
// takes that build's capacities.  Options, slots, the variant table and the choice of a variant are the library's own code and
// tables (csrc/smj_model_load.h, csrc/smj_variants.h, include/smj.h), exported below for tests/emul/emul.py -- nothing is restated here.
#define SMJ_EMUL 1
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../stretch_mujoco_amd/csrc/smj_model_load.h"
#include "../../stretch_mujoco_amd/csrc/smj_step_impl.h"
#include "../../stretch_mujoco_amd/csrc/smj_variants.h"
#include "../host_uploader.h"

struct emul_ctx {
  DevModel m{};
  DevState s{};
  std::vector<void*> keep;
  std::string err;
  struct { Smem s; unsigned char pgs_tail[sizeof(float) * (NEFC * (NEFC + 1) / 2 + NEFP * NEFP)]; } lds;   // PGS: A runs past the end of Smem
};

extern "C" {

emul_ctx* emul_create(const void* blob, size_t nbytes, int num_envs) {
  emul_ctx* c = new emul_ctx();
  HostUploader up{&c->keep};
  const SmjCaps caps{NVP, NBP, NENT, NEFC, NCON, NVS, NSAT};   // this build's capacities (Makefile: -DSMJ_BUILD_TAG=<tag>)
  int chosen = 0;
  if (smj_load_model(blob, nbytes, c->m, up, c->err, &caps, 1, &chosen)) {
    fprintf(stderr, "emul_create: %s\n", c->err.c_str());
    delete c;
    return nullptr;
  }
  c->s.B = num_envs;
  c->s.ld = num_envs;
  c->s.lay = smj_stage_layout(NVP, NBT, NSAT);
  c->s.sepcache = (float*)calloc((size_t)num_envs * SMJ_SEP_SLOTS * 4, sizeof(float));
  c->keep.push_back(c->s.sepcache);
  c->s.mcache = (float*)calloc((size_t)num_envs * SMJ_MC_SLOTS * SMJ_MC_WORDS, sizeof(float));
  c->keep.push_back(c->s.mcache);
  c->s.pgsprev = (float*)calloc((size_t)num_envs * SMJ_PGSPREV_STRIDE, sizeof(float));
  c->keep.push_back(c->s.pgsprev);
  return c;
}
// what smj_reset drops of the library's own memory (smj_kernels.hip smj_reset_kernel): kept manifolds, separating directions, PGS second start
void emul_clear_caches(emul_ctx* c) {
  const size_t B = (size_t)c->s.B;
  memset(c->s.sepcache, 0, B * SMJ_SEP_SLOTS * 4 * sizeof(float));
  memset(c->s.mcache, 0, B * SMJ_MC_SLOTS * SMJ_MC_WORDS * sizeof(float));
  memset(c->s.pgsprev, 0, B * SMJ_PGSPREV_STRIDE * sizeof(float));
}
void emul_destroy(emul_ctx* c) {
  for (void* p : c->keep) free(p);
  delete c;
}
int emul_bind(emul_ctx* c, int slot, void* p, long ld) {   // slot: SMJ_SLOT_* (include/smj.h)
  c->s.ld = ld;
  return smj_bind_slot(c->s, slot, p) ? 0 : -1;
}
// the contact-readout slot (SMJ_SLOT_CONTACTS): env-major records [B][cap][SMJ_CR_WORDS], cap >= the build's NCON
int emul_bind_contacts(emul_ctx* c, void* p, int cap) {
  if (p && cap < NCON) return -1;
  c->s.contacts = (float*)p;
  c->s.con_cap = cap;
  return 0;
}
int emul_contact_words() { return SMJ_CR_WORDS; }
int emul_set_option(emul_ctx* c, const char* name, double v) {
  DevModel& m = c->m;
  if (smj_set_solver_option(m, name, v)) return 0;   // the library's list (SMJ_SOLVER_OPTIONS)
  // emulator only: two fields the library never takes by name.  pgs_cap is what smj_step_tu.h sets itself for a PGS launch without
  // dynamic LDS; multi_serial keeps the serial multiccd search as the comparator of the batched one.
  if (!strcmp(name, "pgs_cap")) m.pgs_cap = (int)v;
  else if (!strcmp(name, "multi_serial")) m.multi_serial = (int)v;
  else return -1;
  return 0;
}
// LDS is uninitialised when a workgroup starts: tests poison the emulated LDS to catch reads before writes
long emul_sep_skips() { return smj_emul_sep_skips; }
long emul_ext_steps() { return smj_emul_ext_steps; }
long emul_mc_hits() { return smj_emul_mc_hits; }
long emul_isl_total() { return smj_emul_isl_total; }
long emul_isl_swept() { return smj_emul_isl_swept; }
int emul_poison = -1;
void emul_set_poison(int byte) { emul_poison = byte; }
int emul_step(emul_ctx* c, int nsteps, unsigned read_flags) {
  for (int env = 0; env < c->s.B; env++) {
    if (emul_poison >= 0) memset(&c->lds, emul_poison, sizeof(c->lds));
    StepKernel* k = new StepKernel(c->m, c->s, c->lds.s, env);
    k->run(nsteps, read_flags);
    delete k;
  }
  return 0;
}
int emul_debug_floats() { return SMJ_DEBUG_FLOATS; }
int emul_nvp() { return NVP; }
int emul_lds_bytes() { return (int)sizeof(Smem); }
int emul_ncon_max() { return NCON; }
int emul_nefc_max() { return NEFC; }
int emul_nsat_max() { return NSAT; }
void emul_caps(SmjCaps* out) { *out = SmjCaps{NVP, NBP, NENT, NEFC, NCON, NVS, NSAT}; }

// ---- the table of variants (csrc/smj_variants.h), the same in every library: row v's name, the tag of its Newton build (whose
// capacities are the variant's), the tag of the build a step beyond them is handed to (null: none)
static const char* const build_tags[SMJ_B_COUNT] = {
#define X(tag) #tag,
    SMJ_BUILDS(X)
#undef X
};
int emul_nvariants() { return SMJ_NVARIANTS; }
const char* emul_variant_name(int v) { return smj_variants[v].name; }
const char* emul_variant_tag(int v) { return build_tags[smj_variants[v].newton]; }
const char* emul_variant_escalation(int v) {
  const SmjVariant& V = smj_variants[v];
  return V.esc_variant != SMJ_NO_VARIANT ? emul_variant_tag(V.esc_variant) : V.esc_build != SMJ_NO_BUILD ? build_tags[V.esc_build] : nullptr;
}
// The row smj_create starts a model on: smj_load_model's choice (smj_pick_variant) among `caps`, the capacities of the table's rows in
// order (each from its own library's emul_caps).  -1: the loader refuses the model.
int emul_pick_variant(const void* blob, size_t nbytes, const SmjCaps* caps, int ncaps) {
  DevModel m{};
  std::vector<void*> keep;
  HostUploader up{&keep};
  std::string err;
  int chosen = -1;
  const int rc = smj_load_model(blob, nbytes, m, up, err, caps, ncaps, &chosen);
  for (void* p : keep) free(p);
  if (rc) fprintf(stderr, "emul_pick_variant: %s\n", err.c_str());
  return rc ? -1 : chosen;
}
}
