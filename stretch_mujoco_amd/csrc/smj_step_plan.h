// HOW A STEP CALL IS LAUNCHED.  smj_builds.h says which builds exist, smj_variants.h which of them a call launches (smj_route); this
// header says how: the host-side scheduling options with their defaults (SmjStepOptions, a member of smj_ctx), the architecture gate of
// smj_create, and ONE pure function, smj_plan_step, that turns the variant, the route, the options and the facts of a call into every
// scheduling decision smj_step and the launchers of smj_step_tu.h carry out.  Plain C++, no HIP types: tests/routing pins it on the CPU.
#pragma once
#include <stddef.h>
#include <string.h>

#include "smj_variants.h"

struct SmjStepOptions {
  int escalate = 1;            // an env whose step needs more rows / contacts than the variant holds is finished by the escalation target
  int balance = 1;             // cost-ordered dispatch: per-env shader time of the last launch, longest first (DevState::order / cost)
  int balance_min = 1;         // steps per launch from which the cost-ordered dispatch is used (round 4: 1 -- a one-step launch is as long as its slowest round of workgroups; was 4)
  int balance_min_envs = 1024; // cost-ordered dispatch only above this many envs
  int pipeline = 5;            // chunk length of the pipelined dispatch (DevState::pipe_len; 0 = one workgroup per env for the whole launch)
  int pipeline_big = 1;        // pipelined dispatch for the two-envs-per-CU builds of the big variant too
  // pipelined chunks (and with them the pollers) only above this many envs (option pipeline_min_envs).  Round 5: 511, was 1024 -- measured under
  // random actions at 1024 envs: empty scene 5.16 -> 5.52 M, kitchen stand-in 3.97 -> 4.98 M, scene.xml 1.96 -> 2.37 M, the kitchen at Robocasa
  // scale 0.73 -> 1.30 M (an env handed to the large build is finished beside the launch instead of after it); at 512 envs nothing but the
  // last (0.56 -> 0.77 M); settled scenes pay 3-5 % for the chunks' state round trips at these sizes
  int pipe_min_envs = 511;
  int pollers = 2;             // tall-variant workgroups that finish parked envs beside the standard kernel (0: the sweep does it all)
  bool pollers_always = false; // option "pollers" < 0: send the pollers with every launch (tests)
  int newton_two_waves = 3;    // Newton on the satellite builds: bit 1 = the 16-satellite family's two-wavefront kernel (smj_kernels_sat2.hip: the second wavefront takes the moving-moving pairs and the satellites' lane-serial stages), bit 2 = the 32-satellite one's; 0 = one wavefront per env
  int pgs_two_waves = 1;       // PGS on the 16-satellite build: 1 = the two-wavefront kernel (smj_kernels_satp.hip), 0 = one wavefront per env
  int lean_build = 1;          // 1 = a call that qualifies (smj_variants.h smj_lean_eligible) runs the lean twin of the standard Newton build, 0 = always the general build (A/B runs, tests), 2 = as 1 with the lean build's twin on the other wavefront count (smj_builds.h SMJ_LEAN_TWIN_BUILDS)
};

// (option name of smj_set_option, field).  All are plain assignments but the two smj_set_step_option spells out.
#define SMJ_STEP_OPTIONS(X)                                                                                                          \
  X("escalate", escalate) X("balance", balance) X("balance_min", balance_min) X("balance_min_envs", balance_min_envs)               \
  X("pipeline", pipeline) X("pipeline_big", pipeline_big) X("pipeline_min_envs", pipe_min_envs) X("pollers", pollers)                \
  X("newton_two_waves", newton_two_waves) X("pgs_two_waves", pgs_two_waves) X("lean_build", lean_build)
static inline bool smj_set_step_option(SmjStepOptions& o, const char* name, double v) {   // false: the list has no option of that name
  if (!strcmp(name, "pollers")) {   // n > 0: n pollers when a recent launch escalated; -n: n pollers with every launch; 0: none
    o.pollers_always = v < 0;
    const int n = (int)(v < 0 ? -v : v);
    o.pollers = n > 256 ? 256 : n;
    return true;
  }
  if (!strcmp(name, "newton_two_waves")) v = (int)v == 1 ? 3 : v;   // 1 (or 3): both satellite builds; 0: neither; tools: 5 = the 16-satellite build only, 2 = the 32-satellite one only
#define X(opt, field) if (!strcmp(name, opt)) { o.field = (int)v; return true; }
  SMJ_STEP_OPTIONS(X)
#undef X
  return false;
}

// The pipelined chunks (and the pollers beside them) lean on workgroups being dispatched in index order: an env's chunk k + 1
// waits -- bounded, 3 s -- for chunk k, which sits B workgroups earlier in the grid.  That holds on the gfx94x / gfx950
// command processors this was measured on; on any other architecture (or when the device's name cannot be read: null) the default
// is the plain launch (one workgroup per env for the whole call).  smj_set_option("pipeline", k) overrides it either way.
static inline void smj_step_options_for_arch(SmjStepOptions& o, const char* gcn_arch_name) {
  if (gcn_arch_name && (!strncmp(gcn_arch_name, "gfx950", 6) || !strncmp(gcn_arch_name, "gfx94", 5))) return;
  o.pipeline = 0;
  o.pollers = 0;
}

// entries of the escalation list a context starts with: a 50-step call is 10 chunks per env; a plan that needs more makes smj_step grow it
static inline size_t smj_redo_initial_cap(int num_envs) { return 16 * (size_t)num_envs; }

struct SmjCallFacts {
  int num_envs, nsteps;
  bool debug_bound, prof_bound;   // SMJ_SLOT_DEBUG / SMJ_SLOT_PROF bound at this call
  bool has_esc;                   // the context holds the escalation model (smj_create: the variant escalates)
};

struct SmjStepPlan {
  bool esc;                // capacity escalation: standard -> tall, big38 / big50 -> big, sat -> sat32
  bool pipe;               // pipelined chunks (DevState::pipe_len) instead of one workgroup per env
  int pipe_len;            // steps per chunk; 0 without pipe
  int pipe_total;          // workgroups of the primary launch = its grid size
  bool clear_sched;        // progress, done_steps and the schedule words are zeroed before the launch
  int redo_need;           // entries the escalation list must hold: every workgroup of the primary launch can park its env once (0: no list)
  bool mark_unpublished;   // the list is filled with -1 = entry not published yet (read by pollers only; a variant that routes none pays the memset unread)
  bool ordered;            // cost-ordered dispatch
  bool poll;               // pollers of the escalation target on the second stream, beside the primary kernel
  int poller_arg;          // DevState::pollers of that launch: the workgroup count, negative = they stay although no recent launch escalated
  int poller_wgs;
  bool sweep;              // the escalation target finishes what is left on the list after the primary kernel
  int sweep_wgs;           // two envs per CU fit (one under PGS); surplus workgroups find the list drained and leave (a launch of one or two steps: 64 -- the empty sweep is pure launch cost there)
};

static inline SmjStepPlan smj_plan_step(const SmjVariant& V, const SmjRoute& route, const SmjStepOptions& o, const SmjCallFacts& f) {
  SmjStepPlan p{};
  const int B = f.num_envs;
  p.esc = f.has_esc && o.escalate;
  // pipelined chunks: batches that need more than one round of workgroups, calls longer than one chunk, neither debug nor profiling slot bound
  const bool pipelines = V.pipelines == SMJ_PIPE_ALWAYS || (V.pipelines == SMJ_PIPE_IF_BIG && o.pipeline_big);
  const int len = V.chunk_len(o.pipeline);
  p.pipe = pipelines && o.pipeline > 0 && f.nsteps > len && !f.debug_bound && !f.prof_bound && B > o.pipe_min_envs;
  p.pipe_len = p.pipe ? len : 0;
  p.pipe_total = B * (p.pipe ? (f.nsteps + len - 1) / len : 1);
  p.clear_sched = p.esc || p.pipe;
  p.redo_need = p.esc ? p.pipe_total : 0;
  p.mark_unpublished = p.esc && p.pipe && o.pollers > 0;
  p.ordered = o.balance && f.nsteps >= o.balance_min && B > o.balance_min_envs;
  // A second kernel resident beside the standard one costs a launch in which nobody escalates 5 % (measured: one poller or
  // sixteen, any poll interval, any stream priority), and escalations are rare events (0-2 envs per 50-step launch of 4096
  // under random actions, each worth milliseconds when left to the sweep): the pollers leave at once unless one of the last
  // SMJ_HOT_LAUNCHES launches had an escalation (DevState::hot, kept on the device -- the host runs many launches ahead)
  p.poll = p.mark_unpublished && route.poller != nullptr;
  p.poller_wgs = V.poller_mult * o.pollers;
  p.poller_arg = o.pollers_always ? -p.poller_wgs : p.poller_wgs;
  p.sweep = p.esc;
  const int sweep_max = f.nsteps <= 2 ? 64 : 512;
  p.sweep_wgs = B < sweep_max ? B : sweep_max;
  return p;
}

// A PGS launch of a primary kernel that can hand steps over (DevState::redo bound, not a worker) keeps to the rows whose A fits the
// struct (rows_static = smj_pgs_rows_static) and asks for no dynamic LDS: the variant's Newton occupancy instead of one env per CU.
// pgs_cap 0: the launch keeps the full LDS and the model's own cap.
struct SmjLdsChoice { size_t lds; int pgs_cap; };
static inline SmjLdsChoice smj_pgs_static_choice(int solver, bool redo_bound, int redo_worker, size_t lds_full, size_t smem_bytes, int rows_static) {
  if (solver != 2 && redo_bound && !redo_worker && lds_full > smem_bytes && rows_static > 0) return {smem_bytes, rows_static};
  return {lds_full, 0};
}
