// Build `sat32n` of the step kernel: what it is stands in the table of smj_builds.h.
#define SMJ_BUILD_TAG sat32n
#include "smj_step_tu.h"
