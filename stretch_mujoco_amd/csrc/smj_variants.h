// THE TABLE OF CAPACITY VARIANTS (smj_ctx::variant, picked by smj_load_model from the model's dimensions) and the one function that
// says which builds of smj_builds.h a step call launches.  Host code without HIP types apart from the launcher pointer inside a
// descriptor: smj_capi.hip includes it, and tests/routing pins it on the CPU.  Second of three headers: smj_builds.h (which builds
// exist), this one (which of them a call launches: smj_route), smj_step_plan.h (how the call launches them: smj_plan_step).
#pragma once
#include "smj_builds.h"

enum { SMJ_NO_BUILD = -1, SMJ_NO_VARIANT = -1 };
enum SmjPipelines { SMJ_PIPE_NEVER = 0, SMJ_PIPE_ALWAYS, SMJ_PIPE_IF_BIG /* when option pipeline_big is set */ };
struct SmjVariant {
  const char* name;
  int newton, pgs;                 // the build that carries each solver (SmjBuildId); its Newton build gives the variant's capacities
  int newton2, newton2_bit;        // Newton on two wavefronts per env, selected by this bit of option newton_two_waves
  int pgs2;                        // PGS on two wavefronts per env, selected by option pgs_two_waves
  int prof;                        // the build launched instead of either when the profiling slot is bound
  int esc_variant, esc_build;      // escalation target: chosen as that variant chooses its primary build | that build; neither: no escalation
  SmjPipelines pipelines;
  int chunk_num, chunk_den;        // chunk length of the pipelined dispatch = ceil(option pipeline * num / den)
  int poller_mult;                 // pollers beside the primary kernel = option pollers * this (0: the sweep does it all)
  bool escalates() const { return esc_variant != SMJ_NO_VARIANT || esc_build != SMJ_NO_BUILD; }
  int chunk_len(int pipeline) const { return (pipeline * chunk_num + chunk_den - 1) / chunk_den; }
};
// Chunk lengths, measured: standard +19 % at chunks of 5, two envs per CU +7 % at 10, three envs per CU chunks of 8 measured 3 % ahead
// of 10, one env per CU (16 rounds of workgroups) nothing.  Pollers: the 16-satellite family hands over to the 32-satellite one the way
// standard hands over to tall; a kitchen's random-action workload parks ~10 envs per launch and each chunk of the large build takes
// milliseconds, hence six times the pollers.
#define B(tag) SMJ_B_##tag
#define NONE SMJ_NO_BUILD
static const SmjVariant smj_variants[7] = {
    //            newton     pgs        newton2    bit pgs2     prof     esc_variant     esc_build pipelines       chunk  pollers
    {"standard", B(step),   B(pgs),    NONE,      0,  NONE,    B(prof), SMJ_NO_VARIANT, B(tall),  SMJ_PIPE_ALWAYS, 1, 1,  1},
    {"mid",      B(mid),    B(midp),   NONE,      0,  NONE,    NONE,    SMJ_NO_VARIANT, B(tall),  SMJ_PIPE_ALWAYS, 3, 2,  0},
    {"big38",    B(big38),  B(big38p), NONE,      0,  NONE,    NONE,    4,              NONE,     SMJ_PIPE_IF_BIG, 2, 1,  0},
    {"big50",    B(big50),  B(big50p), NONE,      0,  NONE,    NONE,    4,              NONE,     SMJ_PIPE_IF_BIG, 2, 1,  0},
    {"big",      B(big),    B(big),    NONE,      0,  NONE,    NONE,    SMJ_NO_VARIANT, NONE,     SMJ_PIPE_NEVER,  1, 1,  0},
    {"sat",      B(sat),    B(sat1),   B(sat2),   1,  B(satp), NONE,    6,              NONE,     SMJ_PIPE_IF_BIG, 2, 1,  6},
    {"sat32",    B(sat32),  B(sat32),  B(sat32n), 2,  NONE,    NONE,    SMJ_NO_VARIANT, NONE,     SMJ_PIPE_NEVER,  1, 1,  0},
};
#undef B
#undef NONE
enum { SMJ_NVARIANTS = sizeof(smj_variants) / sizeof(smj_variants[0]) };

// what one step call launches: the variant's primary kernel; beside it the pollers and after it the sweep of the escalation target
// (null: the variant has none).  no_counters: the profiling slot is bound, the call runs PGS on a variant whose solvers live in
// different builds, and the build it ends in has no cycle counters compiled in (smj_step says so once).
struct SmjRoute { const SmjBuildDesc *primary, *poller, *sweep; bool no_counters; };

// The primary build of variant row `v`; builds[SmjBuildId] = the descriptors of the loaded library.  Selection is by what the
// descriptors say (carries the solver; has counters when the profiling slot is bound), never by launching to find out.
static inline const SmjBuildDesc* smj_primary_build(const SmjVariant& v, int solver, bool prof_bound, int newton_two_waves, int pgs_two_waves,
                                                    const SmjBuildDesc* const* builds) {
  const bool newton = solver == 2;
  if (prof_bound && v.prof != SMJ_NO_BUILD && builds[v.prof]->carries(solver)) return builds[v.prof];
  // two wavefronts per env: not when that would lose the counters the caller asked for
  if (newton && v.newton2 != SMJ_NO_BUILD && (newton_two_waves & v.newton2_bit) && (!prof_bound || builds[v.newton2]->profiling)) return builds[v.newton2];
  if (newton) return builds[v.newton];
  // PGS with the profiling slot bound: a tools library's copy of the Newton-named build keeps both solvers and the counters (big38, big50 of
  // `make bigprof`); the product's carries Newton only, and the PGS twin is what runs
  if (prof_bound && builds[v.newton]->carries(solver) && builds[v.newton]->profiling) return builds[v.newton];
  return builds[v.pgs2 != SMJ_NO_BUILD && pgs_two_waves ? v.pgs2 : v.pgs];
}
static inline SmjRoute smj_route(int variant, int solver, bool prof_bound, int newton_two_waves, int pgs_two_waves, const SmjBuildDesc* const* builds) {
  const SmjVariant& v = smj_variants[variant];
  SmjRoute r{smj_primary_build(v, solver, prof_bound, newton_two_waves, pgs_two_waves, builds), nullptr, nullptr, false};
  r.no_counters = prof_bound && solver != 2 && v.newton != v.pgs && !r.primary->profiling;
  if (v.escalates()) {   // (the escalation model runs with the primary's options: same solver)
    r.sweep = v.esc_variant != SMJ_NO_VARIANT ? smj_primary_build(smj_variants[v.esc_variant], solver, prof_bound, newton_two_waves, pgs_two_waves, builds) : builds[v.esc_build];
    if (v.poller_mult > 0) r.poller = r.sweep;
  }
  return r;
}

// ---- the lean twin of the standard variant's Newton build (smj_builds.h SMJ_ROW_lean, smj_step_impl.h SMJ_LEAN)
// What smj_step knows of ONE call when it chooses between `step` and `lean`: the model's facts (DevModel::nroot), the options as they stand at this call (smj_set_option may have changed them since the last one) and the slots
// bound now.  One field per predicate the lean build folds, plus the switch (option lean_build, default 1; 0: always the general build).
struct SmjLeanFacts {
  int nroot;            // tree roots of the model                         (folded: 1)
  int manifold_cache;   // DevModel::manifold_cache as it stands           (folded: 0)
  bool staged;          // the call runs on the staging rows (DevState::stage)   (folded: yes)
  bool debug_bound;     // SMJ_SLOT_DEBUG is bound                         (folded: no)
  bool prof_bound;      // SMJ_SLOT_PROF is bound: the caller asks for counters, the lean build has none
  int lean_build;       // option lean_build
};
// (templates so that this header stays free of the model's and the state's definitions: Model = DevModel, State = DevState as the call launches it)
template <class Model, class State>
static inline SmjLeanFacts smj_lean_facts(const Model& m, const State& st, int lean_build) {
  return SmjLeanFacts{m.nroot, m.manifold_cache, st.stage != nullptr, st.debug != nullptr, st.prof != nullptr, lean_build};
}
static inline bool smj_lean_eligible(const SmjLeanFacts& f) {
  return f.lean_build != 0 && f.nroot == 1 && f.manifold_cache == 0 && f.staged && !f.debug_bound && !f.prof_bound;
}
// Which lean build a call means: option lean_build = 2 names the twin of smj_builds.h SMJ_LEAN_TWIN_BUILDS (the other wavefront count;
// A/B runs, tests), any other value but 0 the build tagged `lean`.  The result is smj_route_lean's `lean` argument.
static inline const SmjBuildDesc* smj_lean_pick(int lean_build, const SmjBuildDesc* lean, const SmjBuildDesc* twin) { return lean_build == 2 && twin ? twin : lean; }
// The route of a call with the lean twin swapped in where it may run: only for `general` (the standard variant's Newton build -- so
// standard variant, Newton, no satellites, no profiling copy, by what smj_route chose) and only when every folded predicate holds.
// Poller and sweep stay as routed: a step that runs out of rows is handed to the same target.
static inline SmjRoute smj_route_lean(SmjRoute r, const SmjLeanFacts& f, const SmjBuildDesc* general, const SmjBuildDesc* lean) {
  if (lean && r.primary == general && smj_lean_eligible(f)) r.primary = lean;
  return r;
}
