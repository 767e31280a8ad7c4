// Build `lean2` of the step kernel: the lean build on the other wavefront count -- one per env (the table of smj_builds.h; option lean_build = 2).
#define SMJ_BUILD_TAG lean2
#define SMJ_LEAN 1
#include "smj_step_tu.h"
