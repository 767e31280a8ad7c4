// Build `sat2` of the step kernel: what it is stands in the table of smj_builds.h.
#define SMJ_BUILD_TAG sat2
#include "smj_step_tu.h"
