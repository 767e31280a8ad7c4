// What the kernels that store whole grids share (smj_edt.h, smj_nav.h): the qualifier of their inline functions and the arithmetic of
// the store's 16-byte groups.  Compiles under a host compiler like those headers (tests/edt/edt_check.cpp, tests/nav/nav_check.cpp).
// The limits of a kernel (SMJ_EDT_MAX_*, SMJ_NAV_MAX_*, ..) stay in its own header: each follows from that kernel's LDS budget.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SMJ_GRID_HD __host__ __device__ __forceinline__
#else
#define SMJ_GRID_HD static inline
#endif

// The store's 16-byte groups.  A run of n consecutive cells (a row segment of the distance kernel's strip, an env's whole grid in the
// navigation kernel) whose first cell sits `al` words (0 .. 3) past a 16-byte boundary is covered by the groups
// k = 0 .. smj_grid_groups(n) - 1, group k holding the run's cells first .. first + 3 with first = 4 k - al, cut to [0, n): every cell
// is in exactly one group, a group inside the run starts on a 16-byte boundary, and a group with first >= n is empty (the count is
// that of al = 3).
SMJ_GRID_HD int smj_grid_groups(int n) { return (n + 6) >> 2; }
SMJ_GRID_HD int smj_grid_group_first(int k, int al) { return 4 * k - al; }
