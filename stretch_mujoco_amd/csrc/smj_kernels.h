// Launchers of the gfx950 kernels (smj_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smj_model.h"

// One batch-major array [rows][ld] (4-byte words) <-> words off..off+rows of every env's staging row
// (a run of at most 128 rows: one LDS tile per block)
struct StageSeg { void* ptr; int rows, off; };
struct StagePlan {
  StageSeg seg[24];
  int row0[24] = {};   // first row of the run inside its array
  int nseg = 0;
  void add(void* p, int rows, int off) {
    for (int r0 = 0; p && r0 < rows && nseg < 24; r0 += 128) {
      seg[nseg] = StageSeg{p, rows - r0 < 128 ? rows - r0 : 128, off + r0};
      row0[nseg++] = r0;
    }
  }
};

// (the step kernels: one SmjBuildDesc per build, smj_builds.h -- its `launch` is the build's launcher)
void smj_launch_reset(const DevModel& m, const DevState& s, const uint8_t* mask, hipStream_t stream);
// batch-major -> env-major staging rows (import) and back (export); tiles of 64 envs transposed through LDS
void smj_launch_stage(const StagePlan& plan, float* stage, int stride, int B, long ld, bool is_export, hipStream_t stream);
// launch order for the next step launch: envs by descending cost (256 buckets relative to the maximum), one workgroup
void smj_launch_order(const int* cost, int* order, int B, hipStream_t stream);
// one BaseController.update() on the bound BASE_POSE / BASECTL / CTRL arrays (lane = env); the same device function the
// step kernel runs after every step
void smj_launch_base_tick(const DevState& s, hipStream_t stream);
