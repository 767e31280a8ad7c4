// TEST INFRASTRUCTURE ONLY -- the LDS one env of a step-kernel build takes, from the kernel source's own Smem (csrc/smj_step_impl.h) as
// the build's translation unit sees it: compiled HOST-ONLY (no device code is generated) with -DSMJ_BUILD_TAG=<tag> and the switches of
// that unit (-DSMJ_LEAN=1 for the lean builds), for tests/test_lean_two_waves_routing.py.
#define SMJ_STEP_TU 1
#include "smj_builds.h"
#include "smj_step_plan.h"
#include "smj_kernels.h"
#include "smj_step_impl.h"

#include <stdio.h>

int main() {
  printf("tag %s waves %d smem %zu lds_newton %zu w2_collision %d j_offset %zu union_offset %zu\n", SMJ_STR(SMJ_BUILD_TAG), (int)SMJ_BUILD_WAVES, sizeof(Smem),
         smj_lds_bytes(false), (int)SMJ_W2_COLLISION, offsetof(Smem, J), offsetof(Smem, u));
  return 0;
}
