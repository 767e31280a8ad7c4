// TEST INFRASTRUCTURE ONLY -- one build of csrc/smj_builds.h described exactly as its translation unit describes itself (smj_step_tu.h:
// the same initialiser, from the same macros), without compiling the kernel.  The file that includes this defines SMJ_BUILD_TAG,
// PROBE_NAME and, for a profiling copy, SMJ_PROFILING 1 (what `make bigprof` passes with -D).
#define SMJ_STEP_TU 1
#include "smj_builds.h"
#include "smj_model.h"
extern const SmjBuildDesc PROBE_NAME = SMJ_BUILD_DESC_INIT(nullptr);
