/* smj_build.h -- which build of the step kernel a call ran (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI, in a header of its own because existing tests fix the include list and the declarations of smj.h: a caller that
 * wants this entry includes this file (it includes smj.h).  What is declared here is listed in lib.BUILD_EXPORTS.
 */
#ifndef SMJ_BUILD_H
#define SMJ_BUILD_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The tag of the primary step-kernel build the last smj_step of this context launched (csrc/smj_builds.h: "step", "lean", "pgs",
 * "tall", "sat2", ...), "" before the first step.  The library keeps several builds of the same kernel and chooses per call -- by
 * solver, by the slots bound, by options such as newton_two_waves or lean_build; this says which one ran.  Builds of one family give the
 * same results, so nothing but measurements and tests should depend on the answer.  The string is static. */
const char* smj_last_build(const smj_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
