// Build `big50` of the step kernel: what it is stands in the table of smj_builds.h.
#define SMJ_BUILD_TAG big50
#include "smj_step_tu.h"
