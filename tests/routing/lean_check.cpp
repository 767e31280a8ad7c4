// TEST INFRASTRUCTURE ONLY -- which build of the step kernel a step call of a MODEL launches once the lean twin of the standard Newton
// build is in play (csrc/smj_variants.h smj_route_lean), for tests/test_lean_routing.py.  The model blob is loaded by the library's own
// loader among the capacities of the table's rows, the options are set through the library's own list and the slots bound through its
// own switch -- as smj_create / smj_set_option / smj_bind / smj_step do, without a device.  Descriptors: tests/routing/desc_probe.inc.
//   lean_check <blob> [option=value ...] [bind=debug|prof] [lean_build=0|1] [nroot=n] [unstaged]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../host_uploader.h"
#include "smj_model_load.h"
#include "smj_variants.h"

#define X(tag) extern const SmjBuildDesc probe_product_##tag;
SMJ_BUILDS(X)
SMJ_LEAN_BUILDS(X)
#undef X
static const SmjBuildDesc* const builds[SMJ_B_COUNT] = {
#define X(tag) &probe_product_##tag,
    SMJ_BUILDS(X)
#undef X
};

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
  int lean_build = 1;
  for (int a = 2; a < argc; a++) {
    const char* eq = strchr(argv[a], '=');
    const std::string name = eq ? std::string(argv[a], eq - argv[a]) : std::string(argv[a]);
    if (name == "unstaged") st.stage = nullptr;
    else if (name == "bind") {
      if (!smj_bind_slot(st, !strcmp(eq + 1, "debug") ? SMJ_SLOT_DEBUG : SMJ_SLOT_PROF, dummy)) return 2;
    } else if (name == "lean_build") lean_build = atoi(eq + 1);
    else if (name == "nroot" && eq) m.nroot = atoi(eq + 1);   // (no shipped model of the standard variant has a second tree root: the predicate is probed directly)
    else if (!eq || !smj_set_solver_option(m, name.c_str(), atof(eq + 1))) { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  const SmjRoute r0 = smj_route(variant, m.solver, st.prof != nullptr, 3, 1, builds);
  const SmjRoute r = smj_route_lean(r0, smj_lean_facts(m, st, lean_build), builds[SMJ_B_step], &probe_product_lean);
  printf("variant %s general %s primary %s kernel %s poller %s sweep %s same_hand_over %d nroot %d manifold_cache %d\n", smj_variants[variant].name, r0.primary->tag, r.primary->tag,
         r.primary->kernel, r.poller ? r.poller->worker : "-", r.sweep ? r.sweep->worker : "-", (int)(r.poller == r0.poller && r.sweep == r0.sweep), m.nroot, m.manifold_cache);
  for (void* p : keep) free(p);
  return 0;
}
