// Host harness of the base-command arithmetic (stretch_mujoco_amd/csrc/smj_drive.h): the inline functions the HIP kernel calls,
// compiled for the host.  The cell of a point, the swept contribution, the window, the score, the order and the status on their own
// (cases whose answer is read off); then an emulation of the kernel's reductions with the kernel's own functions -- the table pass
// with a per-candidate maximum, the candidate pass with per-thread bests, the butterfly over a wave's 64 lanes and the pass over the
// waves -- for 64, 128 and 256 threads, candidate counts that straddle the wave (1, 2, 63, 64, 65, 130, 1024) and point counts that
// do not divide it, in three orders of the table pass: round by round as the schedule hands the entries out, thread by thread, and
// shuffled.  Each is held against the harness's own double loop, written from the public header's text, on seeded maps whose costs,
// potentials and biases come from small sets, so that equal scores are the rule.  Prints the number of cases and "ok" at the end.
#include "smj_drive.h"
#include "host_check.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

struct Case {
  int nx, ny, K, P, lethal, outside_is_free, goal_weight, obstacle_weight, arrive_potential, own;
  bool have_cost, have_bias, have_twist, pose_finite;
  float v, w, max_dv, max_dw;
  std::vector<int> cells, potential, bias;   // cells [K][P]
  std::vector<uint8_t> cost;
  std::vector<float> command;                // [K][2]
};
struct Result { std::vector<long long> score; int chosen, status; float cmd[2]; };

// ---- long-hand, from the text of include/smj_drive.h
static Result by_definition(const Case& m) {
  Result r;
  r.score.assign(m.K, 0);
  long long best = SMJ_DRIVE_NO_SCORE;
  int at = -1;
  for (int k = 0; k < m.K; k++) {
    bool blocked = false;
    int o = 0;
    for (int p = 0; p + 1 < m.P; p++) {
      const int c = m.cells[k * m.P + p];
      if (c < 0) { if (!m.outside_is_free) blocked = true; continue; }
      const int q = m.have_cost ? m.cost[c] : 0;
      if (q >= m.lethal) blocked = true;
      o = std::max(o, q);
    }
    const int sc = m.cells[k * m.P + m.P - 1];
    long long g = 0;
    if (sc < 0) blocked = true;
    else { g = m.potential[sc]; if (g == (1 << 30)) blocked = true; }
    if (m.have_twist && !(std::fabs(m.command[2 * k] - m.v) <= m.max_dv && std::fabs(m.command[2 * k + 1] - m.w) <= m.max_dw)) blocked = true;
    r.score[k] = blocked ? INT64_MAX : (long long)m.goal_weight * g + (long long)m.obstacle_weight * o + (m.have_bias ? m.bias[k] : 0);
    if (r.score[k] < best) { best = r.score[k]; at = k; }   // strictly smaller: the first of equal scores stays
  }
  if (!m.pose_finite || m.own < 0) r.status = 3;
  else if (m.potential[m.own] <= m.arrive_potential) r.status = 1;
  else if (at < 0) r.status = 2;
  else r.status = 0;
  r.chosen = r.status == 0 ? at : -1;
  r.cmd[0] = r.status == 0 ? m.command[2 * at] : 0.0f;
  r.cmd[1] = r.status == 0 ? m.command[2 * at + 1] : 0.0f;
  return r;
}

// ---- the kernel's phases with the header's functions; order: 0 round by round, 1 thread by thread, 2 shuffled
static Result emulate(const Case& m, int threads, int order, std::mt19937& g) {
  const int K = m.K, P = m.P, n = K * P, rounds = smj_drive_rounds(n, threads);
  std::vector<int> swept(K, 0), goal(K, SMJ_DRIVE_NAV_NONE);
  std::vector<int> visit;
  if (order == 1) {
    for (int t = 0; t < threads; t++)
      for (int r = 0; r < rounds; r++) visit.push_back(r * threads + t);
  } else {
    for (int r = 0; r < rounds; r++)
      for (int t = 0; t < threads; t++) visit.push_back(r * threads + t);
    if (order == 2) std::shuffle(visit.begin(), visit.end(), g);
  }
  int seen = 0;
  for (int i : visit) {
    if (i >= n) continue;
    seen++;
    const int k = i / P, p = i - k * P, at = m.cells[i];
    if (p < P - 1) {
      const int v = smj_drive_swept(at, at >= 0 && m.have_cost ? m.cost[at] : 0, m.lethal, m.outside_is_free);
      if (v > swept[k]) swept[k] = v;   // the LDS atomic max
    } else if (at >= 0) {
      goal[k] = m.potential[at];
    }
  }
  CHECK(seen == n, "the schedule covers %d of %d entries", seen, n);
  Result r;
  r.score.assign(K, 0);
  std::vector<long long> mine(threads, SMJ_DRIVE_NO_SCORE);
  std::vector<int> minek(threads, 0x7fffffff);
  for (int t = 0; t < threads; t++)
    for (int k = t; k < K; k += threads) {
      const bool in = !m.have_twist || smj_drive_in_window(m.command[2 * k], m.command[2 * k + 1], m.v, m.w, m.max_dv, m.max_dw);
      const long long sc = smj_drive_score(swept[k], goal[k], in, m.goal_weight, m.obstacle_weight, m.have_bias ? m.bias[k] : 0);
      r.score[k] = sc;
      if (smj_drive_before(sc, k, mine[t], minek[t])) { mine[t] = sc; minek[t] = k; }
    }
  for (int w0 = 0; w0 < threads; w0 += 64)      // the butterfly: every lane reads its partner's value of the round before
    for (int off = 32; off >= 1; off >>= 1) {
      std::vector<long long> s(mine.begin() + w0, mine.begin() + w0 + 64);
      std::vector<int> q(minek.begin() + w0, minek.begin() + w0 + 64);
      for (int l = 0; l < 64; l++)
        if (smj_drive_before(s[l ^ off], q[l ^ off], mine[w0 + l], minek[w0 + l])) { mine[w0 + l] = s[l ^ off]; minek[w0 + l] = q[l ^ off]; }
    }
  for (int w0 = 0; w0 < threads; w0 += 64)
    for (int l = 1; l < 64; l++) CHECK(mine[w0 + l] == mine[w0] && minek[w0 + l] == minek[w0], "lanes of a wave disagree after the butterfly");
  long long best = mine[0];
  int bestk = minek[0];
  for (int w0 = 64; w0 < threads; w0 += 64)
    if (smj_drive_before(mine[w0], minek[w0], best, bestk)) { best = mine[w0]; bestk = minek[w0]; }
  r.status = smj_drive_status(m.pose_finite, m.own, m.own >= 0 ? m.potential[m.own] : 0, m.arrive_potential, best);
  const bool go = r.status == SMJ_DRIVE_OK;
  r.chosen = go ? bestk : -1;
  r.cmd[0] = go ? m.command[2 * bestk] : 0.0f;
  r.cmd[1] = go ? m.command[2 * bestk + 1] : 0.0f;
  return r;
}

static bool same(const Result& a, const Result& b) {
  return a.score == b.score && a.chosen == b.chosen && a.status == b.status && to_bits(a.cmd[0]) == to_bits(b.cmd[0]) && to_bits(a.cmd[1]) == to_bits(b.cmd[1]);
}

static Case random_case(std::mt19937& g, int nx, int ny, int K, int P, int flavour) {
  Case m;
  const int n = nx * ny;
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
  m.nx = nx; m.ny = ny; m.K = K; m.P = P;
  m.lethal = flavour == 5 ? 256 : 253;
  m.outside_is_free = flavour & 1;
  m.goal_weight = flavour == 6 ? 0 : flavour == 7 ? 65535 : 1;
  m.obstacle_weight = flavour == 6 ? 65535 : flavour == 8 ? 0 : 20;
  m.have_cost = flavour != 2;
  m.have_bias = flavour % 3 == 0;
  m.have_twist = flavour >= 3;
  m.pose_finite = flavour != 9;
  static const int pots[] = {0, 500, 1000, 1500, 1 << 30, (1 << 30) - 1};
  static const int costs[] = {0, 0, 0, 100, 252, 253, 254, 255};
  const int npots = flavour == 4 ? 5 : 4;      // flavour 4 has unreachable cells
  m.potential.resize(n);
  m.cost.resize(n);
  for (int c = 0; c < n; c++) {
    m.potential[c] = pots[pick(0, npots - 1)];
    m.cost[c] = (uint8_t)costs[pick(0, flavour == 10 ? 7 : 4)];      // flavour 10: about 3 in 8 lethal
  }
  if (flavour == 7) m.potential[pick(0, n - 1)] = pots[5];
  m.cells.resize(K * P);
  for (int& c : m.cells) c = pick(0, 19) == 0 ? -1 : pick(0, n - 1);
  if (flavour == 11)                                                    // every candidate blocked: its scoring point is outside
    for (int k = 0; k < K; k++) m.cells[k * P + P - 1] = -1;
  m.bias.resize(K);
  for (int& b : m.bias) b = 500 * pick(-1, 1);
  m.command.resize(2 * K);
  for (int k = 0; k < K; k++) { m.command[2 * k] = 0.05f * (float)(k % 7); m.command[2 * k + 1] = 0.25f * (float)(k % 9 - 4); }
  m.v = flavour == 12 ? NaN : 0.1f; m.w = 0.0f;
  m.max_dv = flavour == 13 ? INF : 0.1f; m.max_dw = flavour == 13 ? INF : 0.5f;
  m.own = flavour == 14 ? -1 : pick(0, n - 1);
  m.arrive_potential = flavour == 15 ? m.potential[m.own >= 0 ? m.own : 0] : 0;      // at its boundary: <= holds with equality
  if (flavour == 15 && m.potential[m.own] >= (1 << 30)) m.potential[m.own] = m.arrive_potential = 1500;
  return m;
}

int main() {
  // ---- the functions on their own
  CHECK(smj_drive_cell(0.0f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4) == 0, "the corner of cell (0, 0) belongs to it");
  CHECK(smj_drive_cell(-1e-6f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4) == -1, "just left of the grid");
  CHECK(smj_drive_cell(0.126f, 0.076f, 0.0f, 0.0f, 0.05f, 4, 4) == 1 * 4 + 2, "cell (2, 1)");
  CHECK(smj_drive_cell(0.2f, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4) == -1 && smj_drive_cell(0.0f, 0.2f, 0.0f, 0.0f, 0.05f, 4, 4) == -1, "the far edges are outside");
  CHECK(smj_drive_cell(-0.974f, -0.974f, -1.0f, -1.0f, 0.05f, 40, 40) == 0, "an origin below zero");
  CHECK(smj_drive_cell(NaN, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4) == -1 && smj_drive_cell(0.0f, INF, 0.0f, 0.0f, 0.05f, 4, 4) == -1 &&
        smj_drive_cell(-INF, 0.0f, 0.0f, 0.0f, 0.05f, 4, 4) == -1 && smj_drive_cell(3e38f, 3e38f, -3e38f, 0.0f, 1e-30f, 4096, 16) == -1, "not finite: outside");
  CHECK(smj_drive_world_x(1.0f, 0.0f, 1.0f, 2.0f, 3.0f) == -2.0f && smj_drive_world_y(1.0f, 0.0f, 1.0f, 2.0f, 3.0f) == 3.0f, "a quarter turn: x forward is +y, y left is -x");
  CHECK(smj_drive_finite(0.0f) && smj_drive_finite(-3.4e38f) && !smj_drive_finite(NaN) && !smj_drive_finite(INF) && !smj_drive_finite(-INF), "finite");
  CHECK(smj_drive_swept(-1, 0, 253, 0) == SMJ_DRIVE_SWEPT_BLOCKS && smj_drive_swept(-1, 0, 253, 1) == 0 && smj_drive_swept(5, 252, 253, 0) == 252 &&
        smj_drive_swept(5, 253, 253, 1) == SMJ_DRIVE_SWEPT_BLOCKS && smj_drive_swept(5, 255, 256, 0) == 255 && smj_drive_swept(5, 0, 1, 0) == 0 &&
        smj_drive_swept(5, 1, 1, 0) == SMJ_DRIVE_SWEPT_BLOCKS, "swept");
  CHECK(smj_drive_in_window(0.2f, 0.5f, 0.1f, 0.0f, 0.1f, 0.5f) && !smj_drive_in_window(0.25f, 0.5f, 0.1f, 0.0f, 0.1f, 0.5f) &&
        !smj_drive_in_window(0.2f, 0.75f, 0.1f, 0.0f, 0.1f, 0.5f) && !smj_drive_in_window(0.2f, 0.5f, NaN, 0.0f, INF, INF) &&
        !smj_drive_in_window(0.2f, 0.5f, 0.1f, NaN, INF, INF) && smj_drive_in_window(0.2f, 0.5f, -7.0f, 9.0f, INF, INF) && smj_drive_in_window(0.2f, 0.5f, 0.2f, 0.5f, 0.0f, 0.0f),
        "window");
  CHECK(smj_drive_score(252, 1000, true, 1, 20, -3) == 1000 + 5040 - 3 && smj_drive_score(256, 1000, true, 1, 20, 0) == SMJ_DRIVE_NO_SCORE &&
        smj_drive_score(0, 1 << 30, true, 1, 20, 0) == SMJ_DRIVE_NO_SCORE && smj_drive_score(0, 0, false, 1, 20, 0) == SMJ_DRIVE_NO_SCORE &&
        smj_drive_score(255, (1 << 30) - 1, true, 65535, 65535, 0x7fffffff) == 65535LL * ((1 << 30) - 1) + 65535LL * 255 + 0x7fffffffLL &&
        smj_drive_score(0, 0, true, 0, 0, -0x7fffffff - 1) == -0x80000000LL, "score");
  CHECK(SMJ_DRIVE_NO_SCORE == INT64_MAX && 65535LL * (1 << 30) + 65535LL * 255 + (1LL << 31) < (1LL << 47), "the bound of the header");
  CHECK(smj_drive_before(1, 9, 2, 0) && !smj_drive_before(2, 0, 1, 9) && smj_drive_before(5, 3, 5, 4) && !smj_drive_before(5, 4, 5, 3) && !smj_drive_before(5, 3, 5, 3) &&
        smj_drive_before(SMJ_DRIVE_NO_SCORE, 0, SMJ_DRIVE_NO_SCORE, 0x7fffffff), "order");
  CHECK(smj_drive_status(false, 3, 0, 100, 5) == SMJ_DRIVE_OFF_GRID && smj_drive_status(true, -1, 0, 100, 5) == SMJ_DRIVE_OFF_GRID &&
        smj_drive_status(true, 3, 100, 100, 5) == SMJ_DRIVE_ARRIVED && smj_drive_status(true, 3, 101, 100, 5) == SMJ_DRIVE_OK &&
        smj_drive_status(true, 3, 100, 100, SMJ_DRIVE_NO_SCORE) == SMJ_DRIVE_ARRIVED && smj_drive_status(true, 3, 101, 100, SMJ_DRIVE_NO_SCORE) == SMJ_DRIVE_BLOCKED &&
        smj_drive_status(true, 3, 1 << 30, (1 << 30) - 1, 7) == SMJ_DRIVE_OK, "status");
  CHECK(smj_drive_rounds(1, 256) == 1 && smj_drive_rounds(256, 256) == 1 && smj_drive_rounds(257, 256) == 2 && smj_drive_rounds(32768, 256) == 128, "rounds");

  // ---- the reductions against the double loop
  std::mt19937 g(20240);
  static const int Ks[] = {1, 2, 63, 64, 65, 130, 1024}, Ps[] = {1, 2, 13, 64, 256}, Ts[] = {64, 128, 256};
  static const int grids[][2] = {{1, 1}, {7, 1}, {16, 12}, {61, 83}};
  int cases = 0, ties = 0, statuses[4] = {0, 0, 0, 0};
  for (int K : Ks)
    for (int P : Ps) {
      if (K * P > SMJ_DRIVE_MAX_TABLE) continue;
      for (int flavour = 0; flavour < 16; flavour++) {
        if (K * P > 8192 && flavour % 4 != 0) continue;      // the large tables: a few flavours
        const int* gr = grids[(flavour + K + P) % 4];
        const Case m = random_case(g, gr[0], gr[1], K, P, flavour);
        const Result want = by_definition(m);
        statuses[want.status]++;
        if (want.chosen >= 0) ties += std::count(want.score.begin(), want.score.end(), want.score[want.chosen]) > 1;
        for (int T : Ts)
          for (int order = 0; order < 3; order++) {
            const Result got = emulate(m, T, order, g);
            CHECK(same(got, want), "K %d P %d flavour %d threads %d order %d: chosen %d status %d, by definition %d %d", K, P, flavour, T, order, got.chosen,
                  got.status, want.chosen, want.status);
            cases++;
          }
      }
    }
  CHECK(ties > 50 && statuses[0] > 50 && statuses[1] > 5 && statuses[2] > 5 && statuses[3] > 5, "vacuous: %d ties, statuses %d %d %d %d", ties, statuses[0], statuses[1],
        statuses[2], statuses[3]);
  printf("%d emulations, %d with a tie for the first place, statuses %d / %d / %d / %d\n", cases, ties, statuses[0], statuses[1], statuses[2], statuses[3]);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
