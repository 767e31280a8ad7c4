// Host harness of the scan-matching arithmetic (stretch_mujoco_amd/csrc/smj_match.h): the inline functions the HIP kernel calls,
// compiled for the host.  The placed test and the cell of a point, the packed word, the shifted cell, the clamp of a bias, the score,
// the index and its inverse, the order, the status and the output pose on their own (cases whose answer is read off); then an
// emulation of the kernel with the kernel's own functions -- the placed points of a rotation as a list of packed words, the candidates of a rotation
// dealt to 64, 128, 256 or 512 threads with per-thread firsts, the butterfly over a wave's 64 lanes and the pass over the waves -- held
// against the harness's own loops, written from the public header's text, on seeded fields from a small set of values, so that equal
// scores are the rule.  Windows 0, 1, 3, 32, rotation counts 1, 5, 64, grids from 1 x 1.  Before those, the split of the field's copy
// into LDS (csrc/smj_scan.h) at every alignment.  Prints the number of cases and "ok".
#include "smj_match.h"
#include "smj_scan.h"
#include "host_check.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Case {
  int nx, ny, T, K, wx, wy, shift_weight, min_points, n;
  bool have_bias, pose_finite;
  float x, y, theta, cell;
  std::vector<int> cells;      // [T][K][2], SMJ_MATCH_NO_CELL twice for none
  std::vector<uint8_t> field;
  std::vector<int> bias;
  std::vector<float> angle;
};
struct Result { std::vector<int> score; int best[4]; float pose[3]; };

// ---- long-hand, from the text of include/smj_scanmatch.h
static Result by_definition(const Case& m) {
  Result r;
  const int WX = 2 * m.wx + 1, WY = 2 * m.wy + 1;
  r.score.assign((size_t)m.T * WY * WX, 0);
  long long top = -(1LL << 40);
  int at = -1;
  for (int t = 0; t < m.T; t++)
    for (int dy = -m.wy; dy <= m.wy; dy++)
      for (int dx = -m.wx; dx <= m.wx; dx++) {
        long long S = 0;
        for (int k = 0; k < m.K; k++) {
          const int ix = m.cells[(t * m.K + k) * 2], iy = m.cells[(t * m.K + k) * 2 + 1];
          if (ix == -32768) continue;
          const int sx = ix + dx, sy = iy + dy;
          if (sx >= 0 && sx < m.nx && sy >= 0 && sy < m.ny) S += m.field[sy * m.nx + sx];
        }
        long long b = m.have_bias ? m.bias[t] : 0;
        b = std::min(std::max(b, 0LL), 1LL << 20);
        const long long J = S - b - (long long)m.shift_weight * (dx * dx + dy * dy);
        const int i = (t * WY + (dy + m.wy)) * WX + (dx + m.wx);
        r.score[i] = (int)J;
        if (J > top) { top = J; at = i; }   // strictly larger: the first of equal scores stays
      }
  const int status = !m.pose_finite ? 2 : m.n < m.min_points ? 1 : 0;
  r.best[0] = status == 0 ? at : -1;
  r.best[1] = status == 0 ? (int)top : 0;
  r.best[2] = m.n;
  r.best[3] = status;
  r.pose[0] = m.x; r.pose[1] = m.y; r.pose[2] = m.theta;
  if (status == 0) {
    const int dx = at % WX - m.wx, dy = (at / WX) % WY - m.wy, t = at / (WX * WY);
    r.pose[0] = std::fmaf((float)dx, m.cell, m.x);
    r.pose[1] = std::fmaf((float)dy, m.cell, m.y);
    r.pose[2] = m.theta + m.angle[t];
  }
  return r;
}

// ---- the kernel's phases with the header's functions
static Result emulate(const Case& m, int threads) {
  Result r;
  const int wx = m.wx, wy = m.wy, WX = 2 * wx + 1, C = WX * (2 * wy + 1);
  r.score.assign((size_t)m.T * C, 0);
  std::vector<int> mineJ(threads, -0x7fffffff - 1), minei(threads, 0x7fffffff), word;
  for (int t = 0; t < m.T; t++) {
    word.clear();      // the list of placed points, in an order of its own: the LDS atomic hands out the slots as the lanes come
    for (int k = m.K - 1; k >= 0; k--)
      if (m.cells[(t * m.K + k) * 2] != SMJ_MATCH_NO_CELL) word.push_back(smj_match_pack(m.cells[(t * m.K + k) * 2], m.cells[(t * m.K + k) * 2 + 1]));
    const int bias = smj_match_bias(m.have_bias ? m.bias[t] : 0);
    for (int tid = 0; tid < threads; tid++)
      for (int cand = tid; cand < C; cand += threads) {
        const int dyi = cand / WX, dx = cand - dyi * WX - wx, dy = dyi - wy;
        int S = 0;
        for (size_t k = 0; k < word.size(); k++) {
          const int at = smj_match_shifted(smj_match_pack_x(word[k]), smj_match_pack_y(word[k]), dx, dy, m.nx, m.ny);
          S += at >= 0 ? (int)m.field[at] : 0;
        }
        const int J = smj_match_score(S, bias, m.shift_weight, dx, dy), i = smj_match_index(t, dy, dx, wx, wy);
        CHECK(i == t * C + cand, "index %d of candidate %d of rotation %d", i, cand, t);
        r.score[i] = J;
        if (smj_match_before(J, i, mineJ[tid], minei[tid])) { mineJ[tid] = J; minei[tid] = i; }
      }
  }
  for (int w0 = 0; w0 < threads; w0 += 64)      // the butterfly: every lane reads its partner's value of the round before
    for (int off = 32; off >= 1; off >>= 1) {
      std::vector<int> s(mineJ.begin() + w0, mineJ.begin() + w0 + 64), q(minei.begin() + w0, minei.begin() + w0 + 64);
      for (int l = 0; l < 64; l++)
        if (smj_match_before(s[l ^ off], q[l ^ off], mineJ[w0 + l], minei[w0 + l])) { mineJ[w0 + l] = s[l ^ off]; minei[w0 + l] = q[l ^ off]; }
    }
  for (int w0 = 0; w0 < threads; w0 += 64)
    for (int l = 1; l < 64; l++) CHECK(mineJ[w0 + l] == mineJ[w0] && minei[w0 + l] == minei[w0], "lanes of a wave disagree after the butterfly");
  int J = mineJ[0], i = minei[0];
  for (int w0 = 64; w0 < threads; w0 += 64)
    if (smj_match_before(mineJ[w0], minei[w0], J, i)) { J = mineJ[w0]; i = minei[w0]; }
  const int status = smj_match_status(m.pose_finite, m.n, m.min_points);
  const bool ok = status == SMJ_MATCH_OK;
  int t, dy, dx;
  smj_match_unindex(i, wx, wy, &t, &dy, &dx);
  CHECK(t >= 0 && t < m.T && dy >= -wy && dy <= wy && dx >= -wx && dx <= wx && smj_match_index(t, dy, dx, wx, wy) == i, "the inverse of index %d", i);
  r.pose[0] = ok ? smj_match_pose_xy(dx, m.cell, m.x) : m.x;
  r.pose[1] = ok ? smj_match_pose_xy(dy, m.cell, m.y) : m.y;
  r.pose[2] = ok ? smj_match_pose_theta(m.theta, m.angle[t]) : m.theta;
  r.best[0] = ok ? i : -1;
  r.best[1] = ok ? J : 0;
  r.best[2] = m.n;
  r.best[3] = status;
  return r;
}

static bool same(const Result& a, const Result& b) {
  return a.score == b.score && std::equal(a.best, a.best + 4, b.best) && to_bits(a.pose[0]) == to_bits(b.pose[0]) && to_bits(a.pose[1]) == to_bits(b.pose[1]) &&
         to_bits(a.pose[2]) == to_bits(b.pose[2]);
}

static Case random_case(std::mt19937& g, int nx, int ny, int T, int K, int wx, int wy, int flavour) {
  Case m;
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
  m.nx = nx; m.ny = ny; m.T = T; m.K = K; m.wx = wx; m.wy = wy;
  m.shift_weight = flavour == 1 ? 1024 : flavour == 2 ? 3 : 0;
  m.have_bias = flavour % 3 == 0;
  m.pose_finite = flavour != 4;
  m.min_points = flavour == 5 ? K + 1 : 1;
  m.n = K;
  m.x = flavour == 4 ? NaN : 0.3125f; m.y = -1.7f; m.theta = 0.4f; m.cell = 0.05f;
  static const uint8_t values[] = {0, 0, 255, 200, 13};
  m.field.resize((size_t)nx * ny);
  for (uint8_t& v : m.field) v = flavour == 6 ? 255 : values[pick(0, 4)];      // flavour 6: every candidate on the grid ties
  m.cells.resize((size_t)T * K * 2);
  for (int j = 0; j < T * K; j++) {
    const bool none = pick(0, 9) == 0;
    m.cells[2 * j] = none ? SMJ_MATCH_NO_CELL : pick(-32, nx + 31);
    m.cells[2 * j + 1] = none ? SMJ_MATCH_NO_CELL : pick(-32, ny + 31);
  }
  static const int biases[] = {0, 0, 255, -5, 1 << 21, 1 << 20};
  m.bias.resize(T);
  for (int& b : m.bias) b = biases[pick(0, 5)];
  m.angle.resize(T);
  for (int t = 0; t < T; t++) m.angle[t] = 0.0087f * (float)((t + 1) / 2) * (t % 2 ? -1.0f : 1.0f);
  return m;
}

int main() {
  // ---- the functions on their own
  int ix, iy;
  CHECK(smj_match_placed(-32.0f, 0.0f, 4, 4) && !smj_match_placed(-33.0f, 0.0f, 4, 4) && smj_match_placed(35.0f, 35.0f, 4, 4) && !smj_match_placed(36.0f, 0.0f, 4, 4) &&
        !smj_match_placed(0.0f, 36.0f, 4, 4) && !smj_match_placed(0.0f, -33.0f, 4, 4), "the band of 32 cells");
  CHECK(!smj_match_placed(NaN, 0.0f, 4, 4) && !smj_match_placed(0.0f, NaN, 4, 4) && !smj_match_placed(INF, 0.0f, 4, 4) && !smj_match_placed(0.0f, -INF, 4, 4) &&
        !smj_match_placed(3e38f, 0.0f, 4096, 16), "not finite, or beyond any int: not placed");
  CHECK(smj_match_floor(0.126f, 0.0f, 0.05f) == 2.0f && smj_match_floor(-1e-6f, 0.0f, 0.05f) == -1.0f && smj_match_floor(-0.974f, -1.0f, 0.05f) == 0.0f, "the float index");
  CHECK(smj_match_cell(0.0f, 0.0f, 1.0f, 0.0f, 0.126f, 0.076f, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == 2 && iy == 1, "cell (2, 1)");
  CHECK(smj_match_cell(1.0f, 1.0f, 0.0f, 1.0f, 2.0f, 3.0f, 0.0f, 0.0f, 1.0f, 8, 8, &ix, &iy) && ix == -2 && iy == 3, "a quarter turn: x forward is +y, y left is -x");
  CHECK(smj_match_cell(0.0f, 0.0f, 1.0f, 0.0f, -1.6f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == -32 && iy == 0, "the band's first column");
  CHECK(!smj_match_cell(0.0f, 0.0f, 1.0f, 0.0f, -1.66f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == SMJ_MATCH_NO_CELL && iy == SMJ_MATCH_NO_CELL, "beyond the band");
  CHECK(!smj_match_cell(NaN, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == SMJ_MATCH_NO_CELL && iy == SMJ_MATCH_NO_CELL, "a pose that is not finite");
  CHECK(!smj_match_cell(0.0f, 0.0f, 1.0f, 0.0f, NaN, NaN, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == SMJ_MATCH_NO_CELL, "a ray without a return keeps NaN");
  for (int a : {-32768, -32, -1, 0, 1, 4095, 4127})
    for (int b : {-32768, -32, -1, 0, 1, 4095, 4127}) {
      const int w = smj_match_pack(a, b);
      CHECK(smj_match_pack_x(w) == a && smj_match_pack_y(w) == b, "pack (%d, %d)", a, b);
    }
  CHECK(smj_match_shifted(0, 0, 0, 0, 4, 3) == 0 && smj_match_shifted(3, 2, 0, 0, 4, 3) == 11 && smj_match_shifted(3, 2, 1, 0, 4, 3) == -1 && smj_match_shifted(3, 2, 0, 1, 4, 3) == -1 &&
        smj_match_shifted(-32, -32, 32, 32, 4, 3) == 0 && smj_match_shifted(35, 34, -32, -32, 4, 3) == 11 && smj_match_shifted(-1, 0, 0, 0, 4, 3) == -1, "the shifted cell");
  for (int d = -32; d <= 32; d++)
    CHECK(smj_match_shifted(SMJ_MATCH_NO_CELL, SMJ_MATCH_NO_CELL, d, d, 4096, 16) == -1 && smj_match_shifted(SMJ_MATCH_NO_CELL, SMJ_MATCH_NO_CELL, d, -d, 16, 4096) == -1,
          "no cell stays off every grid at shift %d", d);
  CHECK(smj_match_bias(-1) == 0 && smj_match_bias(0) == 0 && smj_match_bias(77) == 77 && smj_match_bias(1 << 20) == 1 << 20 && smj_match_bias((1 << 20) + 1) == 1 << 20 &&
        smj_match_bias(0x7fffffff) == 1 << 20 && smj_match_bias(-0x7fffffff - 1) == 0, "the clamp of a bias");
  CHECK(smj_match_score(1000, 7, 3, -2, 1) == 1000 - 7 - 15 && smj_match_score(0, 1 << 20, 1024, 32, -32) == -(1 << 20) - (1 << 21) && smj_match_score(0, 1 << 20, 1024, 32, -32) > -(1 << 22) &&
        1024 * 255 < 1 << 18, "the score and the bounds of the header");
  CHECK(smj_match_index(0, 0, 0, 0, 0) == 0 && smj_match_index(0, -2, -3, 3, 2) == 0 && smj_match_index(0, -2, -2, 3, 2) == 1 && smj_match_index(0, -1, -3, 3, 2) == 7 &&
        smj_match_index(1, -2, -3, 3, 2) == 35 && smj_match_index(63, 32, 32, 32, 32) == 64 * 65 * 65 - 1, "the index");
  CHECK(smj_match_before(2, 9, 1, 0) && !smj_match_before(1, 0, 2, 9) && smj_match_before(5, 3, 5, 4) && !smj_match_before(5, 4, 5, 3) && !smj_match_before(5, 3, 5, 3) &&
        smj_match_before(-(1 << 22), 0, -0x7fffffff - 1, 0x7fffffff), "order");
  CHECK(smj_match_status(false, 1000, 1) == SMJ_MATCH_OFF && smj_match_status(true, 29, 30) == SMJ_MATCH_FEW && smj_match_status(true, 30, 30) == SMJ_MATCH_OK &&
        smj_match_status(false, 0, 30) == SMJ_MATCH_OFF && smj_match_status(true, 0, 1) == SMJ_MATCH_FEW, "status");
  CHECK(to_bits(smj_match_pose_xy(3, 0.05f, 0.3125f)) == to_bits(std::fmaf(3.0f, 0.05f, 0.3125f)) && smj_match_pose_xy(0, 0.05f, -1.7f) == -1.7f &&
        smj_match_pose_theta(0.4f, -0.0087f) == 0.4f + -0.0087f, "the output pose");
  {
    const float o[2] = {0.25f, -0.5f}, d[2] = {0.5f, 2.0f};
    float p[2];
    smj_match_point(o, d, 1.5f, p);
    CHECK(p[0] == 1.0f && p[1] == 2.5f, "the end of a ray");
    float len;
    CHECK(smj_occ_classify(1.0f, 0.2f, 5.0f, 0, &len) == SMJ_OCC_RETURN && len == 1.0f && smj_occ_classify(-1.0f, 0.2f, 5.0f, 0, &len) == SMJ_OCC_DROP &&
          smj_occ_classify(NaN, 0.2f, 5.0f, 0, &len) == SMJ_OCC_DROP && smj_occ_classify(0.1f, 0.2f, 5.0f, 0, &len) == SMJ_OCC_DROP &&
          smj_occ_classify(INF, 0.2f, 5.0f, 0, &len) == SMJ_OCC_DROP, "only a return counts");
  }

  check_stage_split<48>(smj_scan_stage_split);      // the copy of the field into LDS, phase (1)

  // ---- the kernel's phases against the loops
  std::mt19937 g(20261);
  static const int windows[][2] = {{0, 0}, {1, 0}, {0, 1}, {3, 2}, {32, 32}}, Ts[] = {1, 5, 64}, threads[] = {64, 128, 256, 512};
  static const int grids[][2] = {{1, 1}, {7, 1}, {16, 12}, {61, 83}};
  int cases = 0, ties = 0, statuses[3] = {0, 0, 0};
  for (const int* w : windows)
    for (int T : Ts)
      for (int flavour = 0; flavour < 7; flavour++) {
        if (w[0] == 32 && (T == 64 || flavour % 3 != 0)) continue;      // the widest window: a few flavours
        const int* gr = grids[(flavour + T + w[0]) % 4];
        const Case m = random_case(g, gr[0], gr[1], T, w[0] == 32 ? 37 : 1 + 19 * (flavour % 4), w[0], w[1], flavour);
        const Result want = by_definition(m);
        statuses[want.best[3]]++;
        if (want.best[0] >= 0) ties += std::count(want.score.begin(), want.score.end(), want.best[1]) > 1;
        for (int th : threads) {
          const Result got = emulate(m, th);
          CHECK(same(got, want), "window %d x %d T %d flavour %d threads %d: best %d %d %d %d, by definition %d %d %d %d", w[0], w[1], T, flavour, th, got.best[0],
                got.best[1], got.best[2], got.best[3], want.best[0], want.best[1], want.best[2], want.best[3]);
          cases++;
        }
      }
  CHECK(ties > 20 && statuses[0] > 40 && statuses[1] > 5 && statuses[2] > 5, "vacuous: %d ties, statuses %d %d %d", ties, statuses[0], statuses[1], statuses[2]);
  printf("%d emulations, %d with a tie for the first place, statuses %d / %d / %d\n", cases, ties, statuses[0], statuses[1], statuses[2]);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
