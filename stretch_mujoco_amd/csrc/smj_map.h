// A lidar scan into a map at a pose handed in (smj_scan_to_map, include/smj_mapping.h).  The status of an env, the line of a ray laid
// into the map from that pose, what a ray adds to the info counts, and the part of a line's steps whose major coordinate lies inside
// a band, as plain inline functions.  The kernel of smj_map.hip calls exactly these (smj_occ.h for the ray, the classification and the
// closed-form line, smj_match.h for the end of a ray and the float index, smj_drive.h for the transform, smj_hmap.h for the bands);
// the header also compiles under a host compiler, so tests/map/map_check.cpp runs the shipped code serially against its own loops.
//
// The rule.  A ray has its origin o and its end p = o + len d in the robot's frame.  Both are laid into the map from the pose
// (x, y, theta) by the chain the scan matcher uses for a rotation offset of 0 -- smj_drive_world_x / _y, then smj_match_floor -- so
// the end cell of a return is the cell the matcher scored.  The guards of smj_occ_line follow, as float compares before any
// conversion.  From there on everything is integers: the walk is smj_occ_steps / smj_occ_cell / smj_occ_layer as they stand.
#pragma once
#include <math.h>
#include "smj_match.h"   // smj_match_point, smj_match_floor; smj_occ.h (the ray, the line), smj_drive.h (the transform), smj_hmap.h (the bands)

// The rays of a scan (the matcher's limit: its pose is this entry's input).
enum { SMJ_MAP_MAX_RAYS = SMJ_MATCH_MAX_POINTS };
// The public header's macros, token for token, so that a translation unit may include both.
#define SMJ_MAP_OK 0
#define SMJ_MAP_GATED 1
#define SMJ_MAP_OFF 2
#define SMJ_MAP_NO_CELL (-1073741824)
// the words of an env's info
enum { SMJ_MAP_INFO_STATUS = 0, SMJ_MAP_INFO_RETURNS = 1, SMJ_MAP_INFO_CLEARS = 2, SMJ_MAP_INFO_GUARDED = 3 };

// The status of an env: the pose is looked at before the gate.  gate: the env's gate word, 0 without a gate.
SMJ_GRID_HD int smj_map_status(float x, float y, float theta, int gate) {
  if (!(smj_drive_finite(x) && smj_drive_finite(y) && smj_drive_finite(theta))) return SMJ_MAP_OFF;
  return gate != 0 ? SMJ_MAP_GATED : SMJ_MAP_OK;
}

// The line of a ray of kind `kind` (smj_occ_classify) and length len, origin o and direction d in the robot's frame, laid into the
// map from the pose (x, y) with c = cosf(theta), s = sinf(theta).  kind SMJ_OCC_DROP in the result: the ray is not kept.
SMJ_GRID_HD smj_occ_line_t smj_map_line(int kind, const float* o, const float* d, float len, float x, float y, float c, float s, float x0, float y0,
                                        float cell) {
  smj_occ_line_t L = {0, 0, 0, 0, SMJ_OCC_DROP};
  if (kind == SMJ_OCC_DROP) return L;
  float p[2];
  smj_match_point(o, d, len, p);
  const float fax = smj_match_floor(smj_drive_world_x(x, c, s, o[0], o[1]), x0, cell), fay = smj_match_floor(smj_drive_world_y(y, c, s, o[0], o[1]), y0, cell);
  if (!(fabsf(fax) <= 1048576.f && fabsf(fay) <= 1048576.f)) return L;
  const float fbx = smj_match_floor(smj_drive_world_x(x, c, s, p[0], p[1]), x0, cell), fby = smj_match_floor(smj_drive_world_y(y, c, s, p[0], p[1]), y0, cell);
  const float reach = 2.f * (float)SMJ_OCC_MAX_STEPS;
  if (!(fabsf(fbx - fax) <= reach && fabsf(fby - fay) <= reach)) return L;   // differences of integers below 2^22: exact
  L.ax = (int)fax; L.ay = (int)fay;
  L.bx = (int)fbx; L.by = (int)fby;
  L.kind = kind;
  return L;
}

// The word of an env's info that a ray adds 1 to, -1 for none.  cls: what smj_occ_classify made of the range; kept: the kind of the
// ray's line (SMJ_OCC_DROP when a guard dropped it).
SMJ_GRID_HD int smj_map_info_word(int cls, int kept) {
  if (cls == SMJ_OCC_DROP) return -1;
  if (kept == SMJ_OCC_DROP) return SMJ_MAP_INFO_GUARDED;
  return cls == SMJ_OCC_RETURN ? SMJ_MAP_INFO_RETURNS : SMJ_MAP_INFO_CLEARS;
}

// The steps of a line inside a band along the line's MAJOR axis (x when |dx| >= |dy|, as smj_occ_cell has it; n = 0 counts as x).
// There the coordinate of step i is a + i sg with sg = +-1, so the steps with lo <= a + i sg < lo + len are an interval: i_lo .. i_hi
// within 0 .. n, empty when i_lo > i_hi.  Exactly the i for which smj_hmap_slot would not fail on the major coordinate; the minor
// coordinate is still tested per cell.  All values stay below 2^22 in magnitude.
SMJ_GRID_HD void smj_map_range(smj_occ_line_t L, int n, smj_hmap_band_t b, int* i_lo, int* i_hi) {
  const int dx = L.bx - L.ax, dy = L.by - L.ay;
  const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const bool xmajor = adx >= ady;
  const int a = xmajor ? L.ax : L.ay, neg = xmajor ? dx < 0 : dy < 0;
  const int lo = xmajor ? b.c0 : b.r0, hi = lo + (xmajor ? b.cols : b.rows) - 1;   // the band's first and last coordinate
  const int first = neg ? a - hi : lo - a, last = neg ? a - lo : hi - a;
  *i_lo = first > 0 ? first : 0;
  *i_hi = last < n ? last : n;
}

#if defined(__HIPCC__)
// Launch (smj_map.hip).  gate, miss and cell_out may be null.
struct SmjScanSource;   // smj_scan.h
void smj_launch_map(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const float* pose, const int* gate,
                    long gate_ld, float x0, float y0, float cell, int nx, int ny, int no_return_clears, int accumulate, int* hit, int* miss, int* info,
                    int* cell_out, hipStream_t stream);
#endif
