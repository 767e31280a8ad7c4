// What the entries that read the lidar scan share (smj_lidar_to_occupancy, smj_scan_to_pose, smj_scan_to_map, smj_scan_to_particles):
// the source of the rays, the copy of an env's byte field into LDS, the first of a wave in the matcher's order and the store of a
// band.  The split of the field copy is a plain inline function that also compiles under a host compiler, like smj_match.h below it
// (check_stage_split of tests/host_check.h sweeps it, in the match and mcl check programs); the rest is device code for the four kernels.
#pragma once
#include <stdint.h>
#include "smj_match.h"   // smj_match_before; smj_occ.h (the ray, the classification), smj_hmap.h (the split of a band's store) below it

// The copy of ncell bytes from the global address `global_addr` into an LDS array aligned to 16 bytes.  LDS byte sh + i holds byte i,
// so sh + lead is a multiple of 16 in both address spaces: `lead` single bytes up to the first 16-byte boundary, `groups` groups of
// 16 bytes from there (one 16-byte load and store each), single bytes again from byte `tail` on.  Every byte is copied exactly once
// and the last one lands below ncell + 15: the array holds ncell + 16 bytes.
struct smj_scan_split_t { int sh, lead, groups, tail; };

SMJ_GRID_HD smj_scan_split_t smj_scan_stage_split(uintptr_t global_addr, int ncell) {
  smj_scan_split_t s;
  s.sh = (int)(global_addr & 15);
  s.lead = (16 - s.sh) & 15;
  if (s.lead > ncell) s.lead = ncell;
  s.groups = (ncell - s.lead) >> 4;
  s.tail = s.lead + 16 * s.groups;
  return s;
}

#if defined(__HIPCC__)
// Where the rays of a scan come from: the body poses of the XPOSE slot, the model's rangefinder sites and the scan itself.  The first
// member of every scan kernel's argument struct, filled once by the C-ABI (smj_capi.hip scan_source).  The lines that form ray k of
// an env from it (the poses of the site's body and of the frame's body, smj_occ_ray, smj_occ_classify) stay in each kernel: moved
// into a function here they compile to other scalar address arithmetic in all four (profiles/scan_refactor_isa_digest.txt).
struct SmjScanSource {
  const float* xpose;
  long ld;
  const int* lidar_site;
  const int* site_bodyid;
  const float* site_pos;
  const float* site_mat;
  const float* lidar;
  long lidar_ld;
};

// The env's field g[0 .. ncell) into s_raw (aligned to 16 bytes, ncell + 16 bytes) by the split above, bytes as they are; returns
// where field byte 0 sits.  The caller's barrier follows.
template <int THREADS>
__device__ __forceinline__ const uint8_t* smj_scan_stage_field(uint8_t* s_raw, const uint8_t* g, int ncell, int tid) {
  const smj_scan_split_t s = smj_scan_stage_split((uintptr_t)g, ncell);
  uint8_t* dst = s_raw + s.sh;
  for (int i = tid; i < s.lead; i += THREADS) dst[i] = g[i];
  for (int q = tid; q < s.groups; q += THREADS)
    *reinterpret_cast<uint4*>(dst + s.lead + 16 * q) = *reinterpret_cast<const uint4*>(g + s.lead + 16 * q);
  for (int i = s.tail + tid; i < ncell; i += THREADS) dst[i] = g[i];
  return dst;
}

// The first of the wave's 64 (J, i) pairs in the order of smj_match_before, in every lane: a butterfly.  All lanes active.
__device__ __forceinline__ int2 smj_scan_wave_first(int J, int i) {
  for (int off = 32; off >= 1; off >>= 1) {
    const int oJ = __shfl_xor(J, off), oi = __shfl_xor(i, off);
    if (smj_match_before(oJ, oi, J, i)) { J = oJ; i = oi; }
  }
  return make_int2(J, i);
}

// One int32 array of a band, by the split of smj_hmap.h: lead cells, groups of four, the tail.  NULLABLE: src may be null, which
// stores zeros (a kernel that always has a source compiles without the test).
template <int THREADS, bool NULLABLE>
__device__ __forceinline__ void smj_scan_store_band(int* out, const unsigned* src, int ncell, int tid) {
  const smj_hmap_split_t s = smj_hmap_store_split((uintptr_t)out, ncell);
  for (int g = tid; g < s.groups; g += THREADS) {
    const int c = s.lead + 4 * g;
    *reinterpret_cast<int4*>(out + c) = !NULLABLE || src ? make_int4((int)src[c], (int)src[c + 1], (int)src[c + 2], (int)src[c + 3]) : make_int4(0, 0, 0, 0);
  }
  if (tid < s.rest) {   // <= 6 cells
    const int c = smj_hmap_split_rest(s, tid);
    out[c] = !NULLABLE || src ? (int)src[c] : 0;
  }
}
#endif
