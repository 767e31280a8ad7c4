/* smj_localize.h -- where in a map a robot is when nobody knows: Monte Carlo localisation on likelihood fields, the measurement
 * update and the resampling step of a particle filter for the whole batch (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_mapping.h includes this file, smj_scanmatch.h includes that one, and so on up to smj.h, so a caller includes
 * smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the contents of the headers before
 * it; what is declared here is listed in lib.LOCALIZE_EXPORTS and held to the library by tests/test_localize_capi.py.  Same rules as
 * smj.h: caller-owned device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_LOCALIZE_H
#define SMJ_LOCALIZE_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The status of an env: word 3 of its row of stat_dev. */
#define SMJ_MCL_OK 0
#define SMJ_MCL_FEW 1
#define SMJ_MCL_LOST 2

/* Per env P particles -- poses that are NOT a lattice, each with its own sine and cosine -- weighted by the reward the returns of a
 * lidar scan collect from a likelihood field when laid out from the particle, and resampled by those weights.  smj_scan_to_pose
 * searches a window round one prior; this entry carries P hypotheses anywhere on the map, so it finds a robot whose pose is unknown
 * by metres, and its best particle is the prior the matcher then refines.  num_envs and nlidar are the context's; the entry needs
 * SMJ_SLOT_XPOSE bound (the rays' geometry in the robot's frame is read from it) and the model's lidar tables; nlidar <= 1024.  One
 * workgroup per env, no workspace, no global atomics.
 *
 * Inputs.
 * lidar_dev, lidar_ld, frame, r_min, r_max, field_dev, nx, ny, x0, y0, cell: exactly as smj_scan_to_pose takes and refuses them: the
 * scan float32 [nlidar][lidar_ld], range k of env e at k lidar_ld + e; frame a fused body id >= 0; r_min, r_max finite,
 * 0 <= r_min <= r_max, r_max / cell <= 8192; field_dev uint8 [num_envs][ny][nx], any alignment, row-major, rows follow y; nx, ny in
 * [1, 4096] and nx ny <= 65536; cell finite and > 0; x0, y0 finite: the corner of cell (0, 0).
 * particle_dev: float32 [3][num_envs][P], rows x, y, theta in the grid's frame: word j of env e of row q at (q num_envs + e) P + j.
 * P = num_particles in [1, 4096].
 * noise_dev: float32 [3][num_envs][P], or null: what is added to a resampled particle.
 * draw_dev: uint32 [num_envs], one random word per env; required when resample != 0, not read otherwise.
 * span in [1, 262144] (1 << 18); min_points in [1, 1024]; resample in {0, 1}.
 *
 * The points of a scan -- floats, once per env, as smj_scan_to_pose forms them.  Ray k counts when its range is a return
 * (r_min <= r <= r_max); its point is p = o + r d in fp32, with origin o and direction d of the rangefinder in the body `frame`.
 * n is the number of returns whose p is finite.
 *
 * The weight of particle j -- the only other floats.  If x, y or theta of the particle is not finite, S_j = 0.  Otherwise with
 * c = cosf(theta), s = sinf(theta) (the accurate functions) every point gets its cell as smj_scan_to_pose places it at a rotation
 * offset of 0: (gx, gy) = (x + c px - s py, y + s px + c py), fx = floorf((gx - x0) / cell), fy = floorf((gy - y0) / cell), all in
 * fp32, the same operations in the same order; the float compares of that entry decide whether it has a cell, (ix, iy) =
 * ((int)fx, (int)fy).  S_j is the sum of field[iy][ix] over the points whose cell is on the grid, 0 <= ix < nx and 0 <= iy < ny.
 * S_j < 2^18.
 *
 * EVERYTHING BELOW IS INTEGERS.
 * The best particle has the largest S; AMONG EQUAL S THE SMALLEST j WINS.  cut = max(S_max - span, 0); w_j = max(S_j - cut, 0);
 * total = sum of w_j (at most 2^30: int32 holds it); sq = sum of w_j w_j in uint64.
 *
 * Per env the status:
 *   SMJ_MCL_FEW   n < min_points;
 *   SMJ_MCL_LOST  otherwise, S_max == 0: no finite particle puts a return on a rewarded cell;
 *   SMJ_MCL_OK    otherwise.
 * It is word 3 of the env's row of stat_dev: smj_scan_to_map(gate_dev = stat_dev + 3, gate_ld = 8) reads it where it lies, as it
 * reads the matcher's with gate_ld = 4.
 *
 * Resampling -- systematic, and it runs iff resample != 0 and the status is SMJ_MCL_OK.  With r = draw[e], o = ((uint64)r total) >> 32.
 * Slot k has the threshold u_k = ((uint64)k total + o) / P, which is below total for every k.  With the inclusive sums
 * C_j = w_0 + ... + w_j, THE ANCESTOR OF SLOT k IS THE SMALLEST j WITH C_j > u_k; a particle of weight 0 is never an ancestor.
 * particle_out[q][e][k] = particle[q][e][a_k] + noise[q][e][k], one fp32 add per word, or the ancestor's bits as they are when
 * noise_dev is null.  When it does not run, particle_out is the input bit for bit, ancestor[k] = k, and the noise is not read.
 *
 * Outputs.
 * particle_out_dev: float32 [3][num_envs][P], required.
 * weight_dev: int32 [num_envs][P], required: S_j, the raw sum, whatever the status.
 * ancestor_dev: int32 [num_envs][P], or null.
 * stat_dev: int32 [num_envs][8], required: word 0 the best j (-1 unless SMJ_MCL_OK), word 1 S_max, word 2 n, word 3 the status,
 * word 4 total (0 unless OK), word 5 the effective sample size floor(total total / sq), a uint64 division (0 unless OK), word 6 cut,
 * word 7 the number of distinct ancestors (0 when no resampling ran).
 * pose_out_dev: float32 [3][num_envs], or null: with SMJ_MCL_OK the best particle's input pose, bit for bit -- the layout
 * smj_scan_to_pose and smj_scan_to_map take; otherwise all three words hold the bits 0x7FC00000, so every consumer's finite test
 * catches it.
 * A null ancestor_dev or pose_out_dev is left untouched.  Every output word has one value that no order of evaluation changes, so two
 * calls give identical bits; the inputs are unchanged; nothing outside the outputs is written.
 * Errors: -1 for a null lidar_dev / field_dev / particle_dev / particle_out_dev / weight_dev / stat_dev, a null draw_dev with
 * resample != 0, a pointer not aligned to 4 bytes (field_dev excepted), nlidar > 1024, lidar_ld < num_envs, a frame that is no body id
 * or a body id >= nbody, any limit above, an output range that overlaps an input range or another output (the bound SMJ_SLOT_XPOSE is
 * an input: its range runs from its first word to env num_envs-1 of its last row, as the scan's does); -5 when SMJ_SLOT_XPOSE is not
 * bound; -6 for a model without lidar tables.  A refused call writes nothing. */
int smj_scan_to_particles(smj_ctx* ctx, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max,
                          const void* field_dev, int nx, int ny, float x0, float y0, float cell,
                          const void* particle_dev, int num_particles, const void* noise_dev, const void* draw_dev,
                          int span, int min_points, int resample,
                          void* particle_out_dev, void* weight_dev, void* ancestor_dev, void* stat_dev, void* pose_out_dev,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
