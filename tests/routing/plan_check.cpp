// TEST INFRASTRUCTURE ONLY -- prints how a step call is launched (csrc/smj_step_plan.h smj_plan_step) for tests/test_step_plan.py.  The
// arguments are taken in order, as a context lives: the architecture gate first (smj_create), then options by name through the
// library's own list (smj_set_option), slots bound, and every `n=<nsteps>` is one smj_step: it routes (csrc/smj_variants.h), plans,
// prints the plan and grows the escalation list as smj_step does.  Descriptors: tests/routing/desc_probe.inc.  No device.
//   plan_check variant=<name> B=<num_envs> [arch=<gcnArchName>|arch=null] [solver=0|2] [bind=debug|prof] [<option>=<value> ...] n=<nsteps> ...
//   plan_check options [arch=...] [<option>=<value> ...]     the option table as it stands after the arguments
//   plan_check pgs_static <solver> <redo_bound> <redo_worker> <lds_full> <smem_bytes> <rows_static>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "smj_step_plan.h"

#define X(tag) extern const SmjBuildDesc probe_product_##tag;
SMJ_BUILDS(X)
#undef X
static const SmjBuildDesc* const builds[SMJ_B_COUNT] = {
#define X(tag) &probe_product_##tag,
    SMJ_BUILDS(X)
#undef X
};

int main(int argc, char** argv) {
  if (argc >= 8 && !strcmp(argv[1], "pgs_static")) {
    const SmjLdsChoice ch = smj_pgs_static_choice(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]), (size_t)atol(argv[5]), (size_t)atol(argv[6]), atoi(argv[7]));
    printf("lds %zu pgs_cap %d\n", ch.lds, ch.pgs_cap);
    return 0;
  }
  SmjStepOptions opt;
  smj_step_options_for_arch(opt, "gfx950");
  int variant = -1, B = 0, solver = 2;
  bool debug_bound = false, prof_bound = false, only_options = false;
  size_t redo_cap = 0;
  for (int a = 1; a < argc; a++) {
    const char* eq = strchr(argv[a], '=');
    const std::string name = eq ? std::string(argv[a], eq - argv[a]) : std::string(argv[a]);
    const char* val = eq ? eq + 1 : "";
    if (name == "options") only_options = true;
    else if (name == "arch") {   // (a fresh context: the defaults, then the gate)
      opt = SmjStepOptions();
      smj_step_options_for_arch(opt, !strcmp(val, "null") ? nullptr : val);
    } else if (name == "variant") {
      for (int v = 0; v < SMJ_NVARIANTS; v++)
        if (!strcmp(smj_variants[v].name, val)) variant = v;
      if (variant < 0) { fprintf(stderr, "unknown variant %s\n", val); return 2; }
    } else if (name == "B") {
      B = atoi(val);
      redo_cap = smj_redo_initial_cap(B);
    } else if (name == "solver") solver = atoi(val);
    else if (name == "bind") (!strcmp(val, "debug") ? debug_bound : prof_bound) = true;
    else if (name == "n") {
      if (variant < 0 || B <= 0) return 2;
      const SmjVariant& V = smj_variants[variant];
      const SmjCallFacts facts{B, atoi(val), debug_bound, prof_bound, V.escalates()};   // has_esc: smj_create loads the escalation model of a variant that has a target
      const SmjRoute route = smj_route(variant, solver, prof_bound, opt.newton_two_waves, opt.pgs_two_waves, builds);
      const SmjStepPlan p = smj_plan_step(V, route, opt, facts);
      const bool grow = (size_t)p.redo_need > redo_cap;
      printf("has_esc %d esc %d pipe %d pipe_len %d pipe_total %d clear_sched %d redo_need %d redo_cap_before %zu grow %d mark_unpublished %d ordered %d poll %d poller_arg %d "
             "poller_wgs %d sweep %d sweep_wgs %d\n", (int)facts.has_esc, (int)p.esc, (int)p.pipe, p.pipe_len, p.pipe_total, (int)p.clear_sched, p.redo_need, redo_cap, (int)grow,
             (int)p.mark_unpublished, (int)p.ordered, (int)p.poll, p.poller_arg, p.poller_wgs, (int)p.sweep, p.sweep_wgs);
      if (grow) redo_cap = (size_t)p.redo_need;
    } else if (!eq || !smj_set_step_option(opt, name.c_str(), atof(val))) {
      printf("refused %s\n", name.c_str());
      return 3;
    }
  }
  if (only_options) {
#define X(name, field) printf("%s %d ", name, (int)opt.field);
    SMJ_STEP_OPTIONS(X)
#undef X
    printf("pollers_always %d\n", (int)opt.pollers_always);
  }
  return 0;
}
