// Build `lean` of the step kernel: the lean twin of `step` (the table of smj_builds.h; what SMJ_LEAN folds: smj_step_impl.h).
#define SMJ_BUILD_TAG lean
#define SMJ_LEAN 1
#include "smj_step_tu.h"
