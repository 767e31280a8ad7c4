// TEST INFRASTRUCTURE ONLY -- prints what csrc/smj_variants.h routes for every combination tests/test_build_routing.py asks about,
// and the capacities of every build of csrc/smj_builds.h.  Descriptors: tests/routing/desc_probe.inc, one per build and library.
#include <stdio.h>

#include <initializer_list>

#include "smj_variants.h"

#define X(tag) extern const SmjBuildDesc probe_product_##tag, probe_bigprof_##tag;
SMJ_BUILDS(X)
#undef X
static const SmjBuildDesc* const product[SMJ_B_COUNT] = {
#define X(tag) &probe_product_##tag,
    SMJ_BUILDS(X)
#undef X
};
static const SmjBuildDesc* const bigprof[SMJ_B_COUNT] = {
#define X(tag) &probe_bigprof_##tag,
    SMJ_BUILDS(X)
#undef X
};
static const char* worker(const SmjBuildDesc* d) { return !d ? "-" : d->worker ? d->worker : "NO-WORKER"; }

int main() {
  for (int i = 0; i < SMJ_B_COUNT; i++)
    for (const SmjBuildDesc* d : {product[i], bigprof[i]})
      printf("build %s %s family %s caps %d %d %d %d %d %d %d dbg %d solvers %d waves %d profiling %d kernel %s worker %s\n", d == product[i] ? "product" : "bigprof",
             d->tag, d->family, d->caps.nvp, d->caps.nbp, d->caps.nent, d->caps.nefc, d->caps.ncon, d->caps.nvs, d->caps.nsat, d->debug_floats, d->solvers,
             d->waves, d->profiling, d->kernel, d->worker ? d->worker : "-");
  const int n2w_options[4] = {0, 1, 2, 5};
  for (int lib = 0; lib < 2; lib++)
    for (int variant = 0; variant < SMJ_NVARIANTS; variant++)
      for (int solver = 0; solver <= 2; solver += 2)
        for (int prof = 0; prof < 2; prof++)
          for (int n2w_opt : n2w_options)
            for (int p2w = 0; p2w < 2; p2w++) {
              const int n2w = n2w_opt == 1 ? 3 : n2w_opt;   // what smj_set_option stores for option newton_two_waves
              const SmjVariant& V = smj_variants[variant];
              const SmjRoute r = smj_route(variant, solver, prof != 0, n2w, p2w, lib ? bigprof : product);
              if (!r.primary->carries(solver)) { printf("variant %d: primary %s does not carry solver %d\n", variant, r.primary->tag, solver); return 1; }
              printf("route %s %d %d %d %d %d primary %s poller %s sweep %s chunk %d pipelines %d pollers %d no_counters %d\n", lib ? "bigprof" : "product", variant, solver,
                     prof, n2w_opt, p2w, r.primary->kernel, worker(r.poller), worker(r.sweep), V.chunk_len(5), (int)V.pipelines, V.poller_mult * 2, (int)r.no_counters);
            }
  return 0;
}
