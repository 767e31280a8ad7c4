// Host harness of the mapping arithmetic (stretch_mujoco_amd/csrc/smj_map.h): the inline functions the HIP kernel calls, compiled for
// the host.  The status rule, the info word of a ray and the line of a ray with its guards on their own (cases whose answer is read
// off); the band-clipped range of steps against the brute-force set {i : the slot does not fail on the major coordinate} for every
// band of 128 x 96, 37 x 29, 1 x 1, 4096 x 16 and 8192 x 2 and lines in all eight octants, n = 0 and lines wholly off the grid
// included; then an emulation of the kernel with the kernel's own functions -- ray records from float rays, per band the clipped walk
// of groups of 32 lanes, the info counters -- held against the harness's own loops, written from the public header's text.  Prints
// the number of cases and "ok".
#include "smj_map.h"
#include "host_check.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const int GRIDS[][2] = {{128, 96}, {37, 29}, {1, 1}, {4096, 16}, {8192, 2}};

// the slot of a cell whose MINOR coordinate is moved into the band: what is left is the test of the major coordinate
static bool major_inside(smj_hmap_band_t b, bool xmajor, int ix, int iy) { return smj_hmap_slot(b, xmajor ? ix : b.c0, xmajor ? b.r0 : iy) >= 0; }

static long check_range(smj_occ_line_t L, int nx, int ny) {
  const int n = smj_occ_steps(L), dx = L.bx - L.ax, dy = L.by - L.ay;
  const bool xmajor = std::abs(dx) >= std::abs(dy);
  long inside = 0;
  for (int band = 0; band < smj_hmap_bands(nx, ny, SMJ_OCC_BAND_CELLS); band++) {
    const smj_hmap_band_t b = smj_hmap_band(nx, ny, SMJ_OCC_BAND_CELLS, band);
    int lo, hi;
    smj_map_range(L, n, b, &lo, &hi);
    CHECK(lo >= 0 && hi <= n, "range [%d, %d] leaves 0 .. %d", lo, hi, n);
    for (int i = 0; i <= n; i++) {
      int ix, iy;
      smj_occ_cell(L, n, i, &ix, &iy);
      const bool want = major_inside(b, xmajor, ix, iy), got = i >= lo && i <= hi;
      CHECK(want == got, "grid %d x %d band %d line (%d, %d) -> (%d, %d) step %d: in the range %d, by the slot %d", nx, ny, band, L.ax, L.ay, L.bx, L.by, i, (int)got,
            (int)want);
      inside += want;
    }
  }
  return inside;
}

// ---- a scan as the kernel sees it
struct Ray { float o[2], d[2], r; };
struct Scan {
  int nx, ny, no_return_clears, accumulate, gate;
  bool have_miss;
  float x, y, theta, x0, y0, cell, r_min, r_max;
  std::vector<Ray> rays;
  std::vector<int> hit0, miss0;
};
struct Maps { std::vector<int> hit, miss, cells; int info[4]; };

// long-hand, from the text of include/smj_mapping.h
static Maps by_definition(const Scan& m) {
  Maps r;
  const size_t cells = (size_t)m.nx * m.ny;
  const bool finite = std::isfinite(m.x) && std::isfinite(m.y) && std::isfinite(m.theta);
  const int status = !finite ? 2 : m.gate != 0 ? 1 : 0;
  r.info[0] = status; r.info[1] = r.info[2] = r.info[3] = 0;
  r.hit = m.accumulate ? m.hit0 : std::vector<int>(cells, 0);
  r.miss = m.accumulate ? m.miss0 : std::vector<int>(cells, 0);
  r.cells.assign(4 * m.rays.size(), -1073741824);
  if (status != 0) return r;
  const float c = cosf(m.theta), s = sinf(m.theta);
  for (size_t k = 0; k < m.rays.size(); k++) {
    const Ray& q = m.rays[k];
    bool ret = false;
    float len;
    if (q.r != q.r) continue;
    if (q.r >= m.r_min && q.r <= m.r_max) { ret = true; len = q.r; }
    else if (q.r >= 0.f && q.r < m.r_min) continue;
    else if (!m.no_return_clears) continue;
    else len = m.r_max;
    const float px = q.o[0] + len * q.d[0], py = q.o[1] + len * q.d[1];
    const float fax = floorf((m.x + c * q.o[0] - s * q.o[1] - m.x0) / m.cell), fay = floorf((m.y + s * q.o[0] + c * q.o[1] - m.y0) / m.cell);
    const float fbx = floorf((m.x + c * px - s * py - m.x0) / m.cell), fby = floorf((m.y + s * px + c * py - m.y0) / m.cell);
    if (!(fabsf(fax) <= 1048576.f && fabsf(fay) <= 1048576.f && fabsf(fbx - fax) <= 16384.f && fabsf(fby - fay) <= 16384.f)) { r.info[3]++; continue; }
    r.info[ret ? 1 : 2]++;
    const int ax = (int)fax, ay = (int)fay, bx = (int)fbx, by = (int)fby;
    r.cells[4 * k] = ax; r.cells[4 * k + 1] = ay; r.cells[4 * k + 2] = bx; r.cells[4 * k + 3] = by;
    // Bresenham with a running error term
    const int dx = std::abs(bx - ax), dy = std::abs(by - ay), sx = bx < ax ? -1 : 1, sy = by < ay ? -1 : 1, n = std::max(dx, dy);
    int px_ = ax, py_ = ay, err = n;
    for (int i = 0; i <= n; i++) {
      if (px_ >= 0 && px_ < m.nx && py_ >= 0 && py_ < m.ny) (ret && i == n ? r.hit : r.miss)[(size_t)py_ * m.nx + px_]++;
      if (dx >= dy) { px_ += sx; err += 2 * dy; if (err >= 2 * n && n) { err -= 2 * n; py_ += sy; } }
      else { py_ += sy; err += 2 * dx; if (err >= 2 * n) { err -= 2 * n; px_ += sx; } }
    }
  }
  if (!m.have_miss) r.miss = m.miss0;      // a null miss layer is left untouched
  return r;
}

// the kernel's phases with the header's functions, band by band, 256 threads in groups of 32, records in chunks
static Maps emulate(const Scan& m, int chunk) {
  Maps r;
  r.hit = m.hit0; r.miss = m.miss0;
  const int K = (int)m.rays.size(), threads = 256, group = 32;
  r.cells.assign(4 * (size_t)K, 12345);
  const int status = smj_map_status(m.x, m.y, m.theta, m.gate);
  const float c = cosf(m.theta), s = sinf(m.theta);
  for (int band = 0; band < smj_hmap_bands(m.nx, m.ny, SMJ_OCC_BAND_CELLS); band++) {
    const smj_hmap_band_t b = smj_hmap_band(m.nx, m.ny, SMJ_OCC_BAND_CELLS, band);
    const int ncell = b.rows * b.cols;
    const size_t g0 = (size_t)b.r0 * m.nx + b.c0;
    if (status != SMJ_MAP_OK) {
      if (!m.accumulate)
        for (int q = 0; q < ncell; q++) { r.hit[g0 + q] = 0; if (m.have_miss) r.miss[g0 + q] = 0; }
      if (band == 0) {
        r.info[0] = status; r.info[1] = r.info[2] = r.info[3] = 0;
        std::fill(r.cells.begin(), r.cells.end(), SMJ_MAP_NO_CELL);
      }
      continue;
    }
    std::vector<unsigned> hits(ncell), misses(ncell);
    for (int q = 0; q < ncell; q++) { hits[q] = m.accumulate ? (unsigned)m.hit0[g0 + q] : 0u; misses[q] = m.accumulate && m.have_miss ? (unsigned)m.miss0[g0 + q] : 0u; }
    int counts[4] = {0, 0, 0, 0};
    std::vector<smj_occ_line_t> rec(chunk);
    for (int base = 0; base < K; base += chunk) {
      const int count = std::min(chunk, K - base);
      for (int j = 0; j < count; j++) {
        const Ray& q = m.rays[base + j];
        float len;
        const int cls = smj_occ_classify(q.r, m.r_min, m.r_max, m.no_return_clears, &len);
        smj_occ_line_t L = smj_map_line(cls, q.o, q.d, len, m.x, m.y, c, s, m.x0, m.y0, m.cell);
        const int word = smj_map_info_word(cls, L.kind);
        if (word >= 0) counts[word]++;
        if (band == 0) {
          const bool kept = L.kind != SMJ_OCC_DROP;
          const int w[4] = {L.ax, L.ay, L.bx, L.by};
          for (int t = 0; t < 4; t++) r.cells[4 * (size_t)(base + j) + t] = kept ? w[t] : SMJ_MAP_NO_CELL;
        }
        const int xl = std::min(L.ax, L.bx), xh = std::max(L.ax, L.bx), yl = std::min(L.ay, L.by), yh = std::max(L.ay, L.by);
        if (xh < b.c0 || xl >= b.c0 + b.cols || yh < b.r0 || yl >= b.r0 + b.rows) L.kind = SMJ_OCC_DROP;
        rec[j] = L;
      }
      for (int tid = 0; tid < threads; tid++) {
        if (m.have_miss) {
          const int grp = tid / group, lane = tid - grp * group;
          for (int j = grp; j < count; j += threads / group) {
            const smj_occ_line_t L = rec[j];
            if (L.kind == SMJ_OCC_DROP) continue;
            const int n = smj_occ_steps(L);
            int lo, hi;
            smj_map_range(L, n, b, &lo, &hi);
            for (int i = lo + lane; i <= hi; i += group) {
              int ix, iy;
              smj_occ_cell(L, n, i, &ix, &iy);
              const int slot = smj_hmap_slot(b, ix, iy);
              CHECK(slot < ncell, "slot %d of %d", slot, ncell);
              if (slot >= 0) (smj_occ_layer(L, n, i) ? hits : misses)[slot]++;
            }
          }
        } else {
          for (int j = tid; j < count; j += threads) {
            const smj_occ_line_t L = rec[j];
            if (L.kind != SMJ_OCC_RETURN) continue;
            const int slot = smj_hmap_slot(b, L.bx, L.by);
            if (slot >= 0) hits[slot]++;
          }
        }
      }
    }
    for (int q = 0; q < ncell; q++) { r.hit[g0 + q] = (int)hits[q]; if (m.have_miss) r.miss[g0 + q] = (int)misses[q]; }
    if (band == 0) { r.info[0] = SMJ_MAP_OK; for (int t = 1; t < 4; t++) r.info[t] = counts[t]; }
  }
  return r;
}

static Scan random_scan(std::mt19937& g, int nx, int ny, int K, int flavour) {
  Scan m;
  std::uniform_real_distribution<float> u(0.f, 1.f);
  m.nx = nx; m.ny = ny;
  m.cell = 0.05f;
  m.x0 = -0.5f * nx * m.cell + 0.0137f; m.y0 = -0.5f * ny * m.cell - 0.0071f;
  m.x = 0.31f; m.y = -0.17f; m.theta = 6.2f * u(g) - 3.1f;
  m.gate = 0;
  if (flavour == 3) m.theta = NaN;
  if (flavour == 4) m.gate = -3;
  if (flavour == 5) { m.x = INF; m.gate = 1; }
  if (flavour == 6) { m.x = 3000.f; m.y = -3000.f; }      // 3 km off the grid: every cell is skipped
  m.no_return_clears = flavour % 2;
  m.accumulate = (flavour / 2) % 2;
  m.have_miss = flavour != 7;
  m.r_min = 0.2f; m.r_max = flavour == 8 ? 400.f : 5.f;      // 8000 cells: lines far longer than the grid
  static const float bad[] = {NaN, -1.f, 0.1f, 1e9f, INF, -INF};
  for (int k = 0; k < K; k++) {
    Ray q;
    const float a = 6.2831853f * (float)k / (float)K;
    q.o[0] = 0.02f; q.o[1] = -0.01f; q.d[0] = cosf(a); q.d[1] = sinf(a);
    q.r = k % 7 == 3 ? bad[(k / 7) % 6] : m.r_min + (m.r_max - m.r_min) * u(g) * u(g);
    if (k % 41 == 5) q.d[0] = NaN;                          // a ray that fails a guard
    if (k % 41 == 6) { q.d[0] *= 1e6f; q.d[1] *= 1e6f; }    // out of reach
    if (k % 41 == 7) q.o[0] = 1e7f;                         // an origin beyond 2^20 cells
    m.rays.push_back(q);
  }
  std::uniform_int_distribution<int> v(0, 9);
  m.hit0.resize((size_t)nx * ny); m.miss0.resize((size_t)nx * ny);
  for (int& w : m.hit0) w = v(g);
  for (int& w : m.miss0) w = v(g);
  return m;
}

int main() {
  // ---- the functions on their own
  CHECK(smj_map_status(0.f, 0.f, 0.f, 0) == SMJ_MAP_OK && smj_map_status(0.f, 0.f, 0.f, 1) == SMJ_MAP_GATED && smj_map_status(0.f, 0.f, 0.f, -1) == SMJ_MAP_GATED &&
        smj_map_status(0.f, 0.f, 0.f, 2) == SMJ_MAP_GATED && smj_map_status(NaN, 0.f, 0.f, 0) == SMJ_MAP_OFF && smj_map_status(0.f, INF, 0.f, 0) == SMJ_MAP_OFF &&
        smj_map_status(0.f, 0.f, -INF, 0) == SMJ_MAP_OFF && smj_map_status(0.f, 0.f, NaN, 1) == SMJ_MAP_OFF && smj_map_status(3e38f, -3e38f, 1e30f, 0) == SMJ_MAP_OK,
        "the status: the pose before the gate");
  CHECK(smj_map_info_word(SMJ_OCC_DROP, SMJ_OCC_DROP) == -1 && smj_map_info_word(SMJ_OCC_RETURN, SMJ_OCC_RETURN) == 1 && smj_map_info_word(SMJ_OCC_CLEAR, SMJ_OCC_CLEAR) == 2 &&
        smj_map_info_word(SMJ_OCC_RETURN, SMJ_OCC_DROP) == 3 && smj_map_info_word(SMJ_OCC_CLEAR, SMJ_OCC_DROP) == 3, "the info word of a ray");
  CHECK(SMJ_MAP_NO_CELL < -(1 << 21) && SMJ_MAP_MAX_RAYS == 1024, "the constants");
  {
    const float o[2] = {0.5f, 0.f}, d[2] = {1.f, 0.f};
    // a quarter turn at (1, 1): the origin lands at (1, 1.5), the end of length 2 at (1, 3.5)
    smj_occ_line_t L = smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, 1.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.5f);
    CHECK(L.kind == SMJ_OCC_RETURN && L.ax == 2 && L.ay == 3 && L.bx == 2 && L.by == 7, "a quarter turn: (%d, %d) -> (%d, %d)", L.ax, L.ay, L.bx, L.by);
    L = smj_map_line(SMJ_OCC_CLEAR, o, d, 2.f, -1.f, -1.f, 1.f, 0.f, 0.f, 0.f, 0.5f);
    CHECK(L.kind == SMJ_OCC_CLEAR && L.ax == -1 && L.ay == -2 && L.bx == 3 && L.by == -2, "no turn, negative cells: (%d, %d) -> (%d, %d)", L.ax, L.ay, L.bx, L.by);
    int ix, iy;      // the end cell is the matcher's cell of the same point
    CHECK(smj_match_cell(1.f, 1.f, 0.f, 1.f, 2.5f, 0.f, 0.f, 0.f, 0.5f, 64, 64, &ix, &iy) && ix == 2 && iy == 7, "the matcher's cell (%d, %d)", ix, iy);
    CHECK(smj_map_line(SMJ_OCC_DROP, o, d, 2.f, 1.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP, "a dropped range");
    CHECK(smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, NaN, 1.f, 0.f, 1.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP && smj_map_line(SMJ_OCC_RETURN, o, d, NaN, 1.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP &&
          smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, 1.f, 1.f, NaN, NaN, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP && smj_map_line(SMJ_OCC_RETURN, o, d, INF, 1.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP,
          "NaN or infinity anywhere drops the ray");
    CHECK(smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, 524288.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP && smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, 524286.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_RETURN &&
          smj_map_line(SMJ_OCC_RETURN, o, d, 2.f, 0.f, -524290.f, 1.f, 0.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP, "the origin within 2^20 cells");
    CHECK(smj_map_line(SMJ_OCC_RETURN, o, d, 8192.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_RETURN && smj_map_line(SMJ_OCC_RETURN, o, d, 8193.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP &&
          smj_map_line(SMJ_OCC_RETURN, o, d, 8193.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.5f).kind == SMJ_OCC_DROP, "the end within 16384 cells of the origin");
  }

  // ---- the clipped range against the brute-force set
  std::mt19937 g(20262);
  long lines = 0, steps_inside = 0, empty = 0;
  for (const int* gr : GRIDS) {
    const int nx = gr[0], ny = gr[1], many = nx * ny > 20000 ? 60 : 400;
    auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    std::vector<smj_occ_line_t> L;
    for (int sx : {-1, 0, 1})
      for (int sy : {-1, 0, 1})
        for (int major : {0, 1})                                 // eight octants, the axes, the diagonals and n = 0
          for (int t = 0; t < many / 10 + 2; t++) {
            const int big = pick(0, t % 4 == 0 ? 2 * std::max(nx, ny) + 70 : 90), small = pick(0, big);
            const int ax = pick(-40, nx + 40), ay = pick(-40, ny + 40);
            L.push_back({ax, ay, ax + sx * (major ? big : small), ay + sy * (major ? small : big), SMJ_OCC_RETURN});
          }
    for (int t = 0; t < 12; t++) {                               // wholly off the grid, on every side, and through a far corner
      const int far = 100 + 1000 * t;
      L.push_back({-far, -far, -far + 50, -far - 20, SMJ_OCC_CLEAR});
      L.push_back({nx + far, 3, nx + far + 70, 9, SMJ_OCC_CLEAR});
      L.push_back({5, ny + far, -30, ny + far + 33, SMJ_OCC_RETURN});
      L.push_back({-far, ny + far, nx + far, -far, SMJ_OCC_RETURN});
    }
    L.push_back({-8000, 1, 8384, 0, SMJ_OCC_CLEAR});             // 16384 steps, the longest a guard lets through
    L.push_back({3, 8000, 0, -8384, SMJ_OCC_RETURN});
    L.push_back({(1 << 20), (1 << 20), (1 << 20) - 16384, (1 << 20) + 16384, SMJ_OCC_RETURN});
    L.push_back({-(1 << 20), 0, -(1 << 20) + 16384, 7, SMJ_OCC_RETURN});
    for (const smj_occ_line_t& l : L) {
      const long in = check_range(l, nx, ny);
      steps_inside += in;
      empty += in == 0;
      lines++;
    }
  }
  CHECK(steps_inside > 100000 && empty > 100, "vacuous: %ld steps inside a band, %ld lines with none", steps_inside, empty);

  // ---- the kernel's phases against the loops
  int scans = 0, statuses[3] = {0, 0, 0};
  long hits = 0, guarded = 0;
  for (const int* gr : GRIDS)
    for (int flavour = 0; flavour < 9; flavour++) {
      if (gr[0] * gr[1] > 20000 && flavour > 2 && flavour != 8) continue;
      const int K = flavour == 2 ? 1024 : 360;
      const Scan m = random_scan(g, gr[0], gr[1], K, flavour);
      const Maps want = by_definition(m);
      for (int chunk : {384, 1024}) {
        const Maps got = emulate(m, chunk);
        const bool same = got.hit == want.hit && got.miss == want.miss && got.cells == want.cells && std::equal(got.info, got.info + 4, want.info);
        CHECK(same, "grid %d x %d flavour %d chunk %d: info %d %d %d %d, by definition %d %d %d %d", gr[0], gr[1], flavour, chunk, got.info[0], got.info[1], got.info[2],
              got.info[3], want.info[0], want.info[1], want.info[2], want.info[3]);
      }
      statuses[want.info[0]]++;
      guarded += want.info[3];
      if (want.info[0] == 0 && flavour != 6)
        for (size_t q = 0; q < want.hit.size(); q++) hits += want.hit[q] - (m.accumulate ? m.hit0[q] : 0);
      if (flavour == 6) CHECK(want.info[1] > 100 && want.hit == (m.accumulate ? m.hit0 : std::vector<int>(want.hit.size(), 0)), "3 km off: rays kept, no cell touched");
      scans++;
    }
  CHECK(hits > 1000 && guarded > 50 && statuses[0] > 15 && statuses[1] >= 2 && statuses[2] >= 4, "vacuous: %ld hits, %ld guarded, statuses %d %d %d", hits, guarded,
        statuses[0], statuses[1], statuses[2]);
  printf("%ld lines against the brute-force set (%ld steps inside a band, %ld lines with none), %d scans emulated (%ld hits, %ld rays dropped by a guard, statuses %d / %d / %d)\n",
         lines, steps_inside, empty, scans, hits, guarded, statuses[0], statuses[1], statuses[2]);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
