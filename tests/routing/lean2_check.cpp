// TEST INFRASTRUCTURE ONLY -- which lean build a step call of a MODEL launches for each value of option lean_build (csrc/smj_variants.h
// smj_lean_pick + smj_route_lean, called as smj_step calls them), for tests/test_lean_two_waves_routing.py.  As lean_check.cpp: the
// library's own loader, option list and slot switch, no device.  Descriptors: tests/routing/desc_probe.inc.
//   lean2_check <blob> [option=value ...] [bind=debug|prof] [lean_build=0|1|2] [nroot=n] [unstaged]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../host_uploader.h"
#include "smj_model_load.h"
#include "smj_step_plan.h"

#define X(tag) extern const SmjBuildDesc probe_product_##tag;
SMJ_BUILDS(X)
SMJ_LEAN_BUILDS(X)
SMJ_LEAN_TWIN_BUILDS(X)
#undef X
static const SmjBuildDesc* const builds[SMJ_B_COUNT] = {
#define X(tag) &probe_product_##tag,
    SMJ_BUILDS(X)
#undef X
};
// (one tag per list)
#define X(tag) static const SmjBuildDesc* const lean = &probe_product_##tag;
SMJ_LEAN_BUILDS(X)
#undef X
#define X(tag) static const SmjBuildDesc* const twin = &probe_product_##tag;
SMJ_LEAN_TWIN_BUILDS(X)
#undef X

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> blob;
  unsigned char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  std::vector<void*> keep;
  HostUploader up{&keep};
  DevModel m{};
  DevState st{};
  std::string err;
  SmjCaps caps[SMJ_NVARIANTS];
  for (int v = 0; v < SMJ_NVARIANTS; v++) caps[v] = builds[smj_variants[v].newton]->caps;
  int variant = -1;
  if (smj_load_model(blob.data(), blob.size(), m, up, err, caps, SMJ_NVARIANTS, &variant)) { fprintf(stderr, "load: %s\n", err.c_str()); return 1; }
  static float dummy[4];
  st.stage = dummy;   // smj_step runs every call on the staging rows
  SmjStepOptions opt;   // lean_build goes through the library's own option list, as smj_set_option sends it
  for (int a = 2; a < argc; a++) {
    const char* eq = strchr(argv[a], '=');
    const std::string name = eq ? std::string(argv[a], eq - argv[a]) : std::string(argv[a]);
    if (name == "unstaged") st.stage = nullptr;
    else if (name == "bind") {
      if (!smj_bind_slot(st, !strcmp(eq + 1, "debug") ? SMJ_SLOT_DEBUG : SMJ_SLOT_PROF, dummy)) return 2;
    } else if (name == "nroot" && eq) m.nroot = atoi(eq + 1);
    else if (eq && smj_set_step_option(opt, name.c_str(), atof(eq + 1))) continue;
    else if (!eq || !smj_set_solver_option(m, name.c_str(), atof(eq + 1))) { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  const SmjRoute r0 = smj_route(variant, m.solver, st.prof != nullptr, opt.newton_two_waves, opt.pgs_two_waves, builds);
  const SmjRoute r = smj_route_lean(r0, smj_lean_facts(m, st, opt.lean_build), builds[SMJ_B_step], smj_lean_pick(opt.lean_build, lean, twin));
  printf("variant %s general %s primary %s kernel %s waves %d family %s solvers %d poller %s sweep %s same_hand_over %d lean_waves %d twin_waves %d twin_kernel %s lean_kernel %s\n",
         smj_variants[variant].name, r0.primary->tag, r.primary->tag, r.primary->kernel, r.primary->waves, r.primary->family, r.primary->solvers,
         r.poller ? r.poller->worker : "-", r.sweep ? r.sweep->worker : "-", (int)(r.poller == r0.poller && r.sweep == r0.sweep), lean->waves, twin->waves,
         twin->kernel, lean->kernel);
  for (void* p : keep) free(p);
  return 0;
}
