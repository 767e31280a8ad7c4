// Host harness of the particle-filter arithmetic (stretch_mujoco_amd/csrc/smj_mcl.h): the inline functions the HIP kernel calls,
// compiled for the host.  The weight of a point, cut and w, the offset of a draw, the threshold of a slot, the ancestor search, the
// effective sample size and the status on their own (cases whose answer is read off, the extremes of every integer); then an
// emulation of the kernel's integer stage with the kernel's own functions -- particles dealt to 64, 128, 256 or 512 threads with
// per-thread firsts, the butterfly over a wave's 64 lanes and the pass over the waves, the inclusive sums 'threads' at a time (the
// wave's scan as the six lane moves of smj_mcl.hip: shifts by 1, 2, 4, 8 inside a row of 16, the last lane of a row into the next
// row, lane 31 into rows 2 and 3), the carry, the binary search per slot and the rule by which a slot opens a new ancestor -- held
// against the harness's own loops, written from the public header's text, on seeded sums from a small set of values, so that equal
// sums and particles of weight 0 are the rule.  P from 1 to 4096, not only multiples of 64.  Prints the number of cases and "ok".
#include "smj_mcl.h"
#include "smj_scan.h"
#include "host_check.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

struct Case {
  int P, span, min_points, n, resample;
  unsigned draw;
  std::vector<int> S;
};
struct Result { int stat[8]; std::vector<int> ancestor; };

// ---- long-hand, from the text of include/smj_localize.h
static Result by_definition(const Case& m) {
  Result r;
  long long s_max = -1;
  int best = -1;
  for (int j = 0; j < m.P; j++)
    if (m.S[j] > s_max) { s_max = m.S[j]; best = j; }   // strictly larger: the first of equal sums stays
  const int status = m.n < m.min_points ? 1 : s_max == 0 ? 2 : 0;
  const long long cut = std::max(s_max - m.span, 0LL);
  std::vector<long long> w(m.P);
  unsigned long long total = 0, sq = 0;
  for (int j = 0; j < m.P; j++) {
    w[j] = std::max(m.S[j] - cut, 0LL);
    total += (unsigned long long)w[j];
    sq += (unsigned long long)(w[j] * w[j]);
  }
  r.ancestor.resize(m.P);
  for (int k = 0; k < m.P; k++) r.ancestor[k] = k;
  int distinct = 0;
  if (status == 0 && m.resample) {
    const unsigned long long o = ((unsigned long long)m.draw * total) >> 32;
    std::set<int> seen;
    for (int k = 0; k < m.P; k++) {
      const unsigned long long u = ((unsigned long long)k * total + o) / (unsigned long long)m.P;
      unsigned long long C = 0;
      int j = 0;
      for (; j < m.P; j++) {
        C += (unsigned long long)w[j];
        if (C > u) break;
      }
      CHECK(j < m.P && u < total, "slot %d: threshold %llu of total %llu has no ancestor", k, u, total);
      CHECK(j < m.P && w[j] > 0, "slot %d: an ancestor of weight 0", k);
      r.ancestor[k] = j;
      seen.insert(j);
    }
    distinct = (int)seen.size();
  }
  const bool ok = status == 0;
  const int stat[8] = {ok ? best : -1, (int)s_max, m.n, status, ok ? (int)total : 0, ok ? (int)(total * total / sq) : 0, (int)cut, distinct};
  std::copy(stat, stat + 8, r.stat);
  return r;
}

// ---- the wave's inclusive sums by the lane moves of smj_mcl.hip: a lane without a source, or in a masked row, adds 0
static void wave_scan(int* t) {
  int s[64];
  for (int sh : {1, 2, 4, 8}) {      // row_shr: the lane sh below within the row of 16
    std::copy(t, t + 64, s);
    for (int l = 0; l < 64; l++) t[l] += (l & 15) >= sh ? s[l - sh] : 0;
  }
  std::copy(t, t + 64, s);            // row_bcast:15, rows 1 and 3
  for (int l = 0; l < 64; l++) t[l] += (l >> 4) == 1 || (l >> 4) == 3 ? s[(l & ~15) - 1] : 0;
  std::copy(t, t + 64, s);            // row_bcast:31, rows 2 and 3
  for (int l = 0; l < 64; l++) t[l] += (l >> 4) >= 2 ? s[31] : 0;
}

// ---- the kernel's phases with the header's functions
static Result emulate(const Case& m, int threads) {
  Result r;
  const int P = m.P, waves = threads / 64;
  std::vector<int> mineS(threads, -1), minej(threads, 0x7fffffff), s_w(m.S);
  for (int tid = 0; tid < threads; tid++)
    for (int j = tid; j < P; j += threads)
      if (smj_match_before(m.S[j], j, mineS[tid], minej[tid])) { mineS[tid] = m.S[j]; minej[tid] = j; }
  for (int w0 = 0; w0 < threads; w0 += 64)      // the butterfly: every lane reads its partner's value of the round before
    for (int off = 32; off >= 1; off >>= 1) {
      std::vector<int> s(mineS.begin() + w0, mineS.begin() + w0 + 64), q(minej.begin() + w0, minej.begin() + w0 + 64);
      for (int l = 0; l < 64; l++)
        if (smj_match_before(s[l ^ off], q[l ^ off], mineS[w0 + l], minej[w0 + l])) { mineS[w0 + l] = s[l ^ off]; minej[w0 + l] = q[l ^ off]; }
    }
  int s_max = mineS[0], best = minej[0];
  for (int w0 = 64; w0 < threads; w0 += 64)
    if (smj_match_before(mineS[w0], minej[w0], s_max, best)) { s_max = mineS[w0]; best = minej[w0]; }
  const int status = smj_mcl_status(m.n, m.min_points, s_max), cut = smj_mcl_cut(s_max, m.span);
  const bool ok = status == SMJ_MCL_OK;
  r.ancestor.resize(P);
  for (int k = 0; k < P; k++) r.ancestor[k] = k;
  if (!ok) {
    const int stat[8] = {-1, s_max, m.n, status, 0, 0, cut, 0};
    std::copy(stat, stat + 8, r.stat);
    return r;
  }
  int carry = 0;
  uint64_t sq = 0;
  std::vector<int> t(threads), s_wave(waves);
  for (int base = 0; base < P; base += threads) {
    for (int tid = 0; tid < threads; tid++) {
      const int j = base + tid, w = j < P ? smj_mcl_w(s_w[j], cut) : 0;
      sq += (uint64_t)w * (uint64_t)w;
      t[tid] = w;
    }
    for (int wv = 0; wv < waves; wv++) {
      wave_scan(t.data() + 64 * wv);
      s_wave[wv] = t[64 * wv + 63];
    }
    int all = 0;
    for (int wv = 0; wv < waves; wv++) all += s_wave[wv];
    for (int tid = 0; tid < threads; tid++) {
      int before = carry;
      for (int wv = 0; wv < (tid >> 6); wv++) before += s_wave[wv];
      if (base + tid < P) s_w[base + tid] = before + t[tid];
    }
    carry += all;
  }
  const int total = carry;
  int distinct = 0;
  if (m.resample) {
    const unsigned o = smj_mcl_offset(m.draw, total);
    CHECK(o < (unsigned)total, "offset %u of total %d", o, total);
    for (int k = 0; k < P; k++) {
      const int u = smj_mcl_threshold(k, total, o, P), anc = smj_mcl_ancestor(s_w.data(), P, u);
      CHECK(u >= 0 && u < total, "threshold %d of slot %d, total %d", u, k, total);
      distinct += k == 0 || (anc > 0 && smj_mcl_threshold(k - 1, total, o, P) < s_w[anc - 1]);
      r.ancestor[k] = anc;
    }
  }
  const int stat[8] = {best, s_max, m.n, status, total, smj_mcl_ess(total, sq), cut, distinct};
  std::copy(stat, stat + 8, r.stat);
  return r;
}

static Case random_case(std::mt19937& g, int P, int flavour) {
  Case m;
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
  static const unsigned draws[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
  static const int spans[] = {1, 4096, 1 << 18, 300};
  m.P = P;
  m.span = spans[flavour % 4];
  m.n = 360;
  m.min_points = flavour == 5 ? 361 : 30;
  m.resample = flavour != 6;
  m.draw = flavour < 4 ? draws[flavour] : (unsigned)g();
  m.S.resize(P);
  static const int values[] = {0, 0, 91800, 91799, 88000, 5, 1};
  for (int& v : m.S)
    v = flavour == 7 ? 0 : flavour == 8 ? 261120 : flavour == 9 ? pick(0, 261120) : values[pick(0, 6)];      // 7: lost; 8: every particle at the largest sum, ties all the way
  if (flavour == 10) { std::fill(m.S.begin(), m.S.end(), 0); m.S[pick(0, P - 1)] = 17; }                     // one particle on the grid
  return m;
}

int main() {
  check_stage_split<48>(smj_scan_stage_split);      // the copy of the field into LDS, the staged builds' phase (1)

  // ---- the functions on their own
  CHECK(smj_mcl_cut(91800, 4096) == 87704 && smj_mcl_cut(4096, 4096) == 0 && smj_mcl_cut(100, 4096) == 0 && smj_mcl_cut(0, 1) == 0 && smj_mcl_cut(261120, 1) == 261119 &&
        smj_mcl_cut(261120, 1 << 18) == 0, "cut");
  CHECK(smj_mcl_w(91800, 87704) == 4096 && smj_mcl_w(87704, 87704) == 0 && smj_mcl_w(0, 87704) == 0 && smj_mcl_w(5, 0) == 5 && smj_mcl_w(0, 0) == 0, "w");
  CHECK(smj_mcl_offset(0u, 1 << 30) == 0u && smj_mcl_offset(0xFFFFFFFFu, 1 << 30) == (1u << 30) - 1u && smj_mcl_offset(0x80000000u, 7) == 3u && smj_mcl_offset(0xFFFFFFFFu, 1) == 0u &&
        smj_mcl_offset(1u, 1 << 30) == 0u, "the offset of a draw lies below the total");
  CHECK(smj_mcl_threshold(0, 10, 9u, 4) == 2 && smj_mcl_threshold(3, 10, 9u, 4) == 9 && smj_mcl_threshold(4095, 1 << 30, (1u << 30) - 1u, 4096) == (1 << 30) - 1 &&
        smj_mcl_threshold(0, 1, 0u, 1) == 0, "the threshold of a slot lies below the total, in 64 bits");
  {
    const int C[6] = {0, 3, 3, 3, 10, 10};      // w = 0 3 0 0 7 0
    CHECK(smj_mcl_ancestor(C, 6, 0) == 1 && smj_mcl_ancestor(C, 6, 2) == 1 && smj_mcl_ancestor(C, 6, 3) == 4 && smj_mcl_ancestor(C, 6, 9) == 4, "the smallest j with C_j > u");
    const int one[1] = {5};
    CHECK(smj_mcl_ancestor(one, 1, 0) == 0 && smj_mcl_ancestor(one, 1, 4) == 0, "one particle");
  }
  CHECK(smj_mcl_ess(10, 100) == 1 && smj_mcl_ess(10, 50) == 2 && smj_mcl_ess(1 << 30, (uint64_t)4096 << 36) == 4096 && smj_mcl_ess(1, 1) == 1, "the effective sample size");
  CHECK(smj_mcl_status(29, 30, 1000) == SMJ_MCL_FEW && smj_mcl_status(29, 30, 0) == SMJ_MCL_FEW && smj_mcl_status(30, 30, 0) == SMJ_MCL_LOST && smj_mcl_status(30, 30, 1) == SMJ_MCL_OK &&
        smj_mcl_status(0, 1, 5) == SMJ_MCL_FEW, "status: too few returns comes first");
  CHECK(smj_mcl_finite(0.0f, -1.0f, 7.0f) && !smj_mcl_finite(NaN, 0.0f, 0.0f) && !smj_mcl_finite(0.0f, INF, 0.0f) && !smj_mcl_finite(0.0f, 0.0f, -INF), "a particle that is not finite");
  CHECK(4096LL * 360 * 255 <= 1LL << 30 && 1024 * 255 < 1 << 18 && 4096LL * ((1LL << 18) - 1) < 1LL << 30, "the bounds of the header");
  {
    // a 4 x 3 field; a particle at (0.1, 0.1) turned a quarter: x forward is +y
    const uint8_t field[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    CHECK(smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, 0.126f, 0.076f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 7, "cell (2, 1)");
    CHECK(smj_mcl_point_weight(0.01f, 0.01f, 0.0f, 1.0f, 0.1f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 9, "a quarter turn: cell (0, 2)");
    CHECK(smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, 0.21f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0 && smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, -0.01f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0 &&
          smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.16f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0, "inside the band but off the grid reads nothing");
    CHECK(smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, 1e30f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0 && smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, NaN, NaN, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0 &&
          smj_mcl_point_weight(3e38f, -3e38f, 1.0f, 0.0f, 3e38f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 3, field) == 0, "far off, or not a number: never converted");
    // against a loop of its own: points on a lattice of cell centres, a particle that shifts them by whole cells
    int want = 0, got = 0;
    for (int iy = -2; iy < 5; iy++)
      for (int ix = -2; ix < 6; ix++) {
        const int sx = ix + 1, sy = iy - 1;
        if (sx >= 0 && sx < 4 && sy >= 0 && sy < 3) want += field[sy * 4 + sx];
        got += smj_mcl_point_weight(1.0f, -1.0f, 1.0f, 0.0f, (float)ix + 0.5f, (float)iy + 0.5f, 0.0f, 0.0f, 1.0f, 4, 3, field);
      }
    CHECK(got == want && want == 78, "the sum over a lattice of points: %d, by the loop %d", got, want);
  }

  // ---- the kernel's integer stage against the loops
  std::mt19937 g(20262);
  static const int Ps[] = {1, 2, 7, 63, 64, 65, 257, 511, 512, 513, 1000, 1024, 4095, 4096}, threads[] = {64, 128, 256, 512};
  int cases = 0, statuses[3] = {0, 0, 0}, zero_weight = 0, repeated = 0;
  for (int P : Ps)
    for (int flavour = 0; flavour < 11; flavour++) {
      if (P >= 4095 && flavour % 2 == 1 && flavour != 9) continue;      // the long-hand search is quadratic
      const Case m = random_case(g, P, flavour);
      const Result want = by_definition(m);
      statuses[want.stat[3]]++;
      zero_weight += std::count(m.S.begin(), m.S.end(), 0) > 0 && want.stat[3] == 0;
      repeated += want.stat[7] > 0 && want.stat[7] < P;
      for (int k = 1; k < P; k++) CHECK(want.ancestor[k] >= want.ancestor[k - 1], "ancestors are monotone in the slot");
      for (int th : threads) {
        const Result got = emulate(m, th);
        CHECK(std::equal(got.stat, got.stat + 8, want.stat) && got.ancestor == want.ancestor,
              "P %d flavour %d threads %d: stat %d %d %d %d %d %d %d %d, by definition %d %d %d %d %d %d %d %d", P, flavour, th, got.stat[0], got.stat[1], got.stat[2], got.stat[3],
              got.stat[4], got.stat[5], got.stat[6], got.stat[7], want.stat[0], want.stat[1], want.stat[2], want.stat[3], want.stat[4], want.stat[5], want.stat[6], want.stat[7]);
        cases++;
      }
    }
  {
    // the largest total the header allows: 4096 particles of 360 points of 255, span at its cap
    Case m;
    m.P = 4096; m.span = 1 << 18; m.min_points = 1; m.n = 360; m.resample = 1; m.draw = 0xFFFFFFFFu;
    m.S.assign(4096, 360 * 255);
    const Result got = emulate(m, 512);
    CHECK(got.stat[4] == 4096 * 360 * 255 && got.stat[5] == 4096 && got.stat[7] == 4096 && got.stat[0] == 0 && got.ancestor[4095] == 4095 && got.ancestor[17] == 17, "the largest total: %d", got.stat[4]);
    cases++;
  }
  CHECK(statuses[0] > 60 && statuses[1] > 5 && statuses[2] > 5 && zero_weight > 30 && repeated > 30, "vacuous: statuses %d %d %d, %d with particles of weight 0, %d with repeated ancestors",
        statuses[0], statuses[1], statuses[2], zero_weight, repeated);
  printf("%d emulations, statuses %d / %d / %d, %d with particles of weight 0, %d with repeated ancestors\n", cases, statuses[0], statuses[1], statuses[2], zero_weight, repeated);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
