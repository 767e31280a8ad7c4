// Build `prof` of the step kernel: what it is stands in the table of smj_builds.h.
#define SMJ_BUILD_TAG prof
#include "smj_step_tu.h"
