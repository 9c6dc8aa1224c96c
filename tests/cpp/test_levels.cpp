// The level histogram's host arithmetic (scanner_amd/csrc/scn_levels.h: scn_levels_top, scn_levels_level, scn_levels_rank;
// scn_host.hip: check_levels_geometry, check_levels_edges, check_levels_summary, scn_levels_fold_spectrum, scn_levels_merge,
// scn_levels_summary) as a stand-alone program: built by g++ -x c++ together with that unit, no HIP header on the include path, plain
// and under ASan + UBSan (tests/test_levels_cpp.py).  Known answers worked out by hand for n = 16 at 8 MHz with the default mask: the
// evaluated fftshift indices are i in {2, 3, 4, 12, 13, 14} (natural bins j = 10, 11, 12, 4, 5, 6), bin_step = 500000, and a unit
// centred at 100 MHz has its evaluated bins at 97.0, 97.5, 98.0, 102.0, 102.5 and 103.0 MHz.  Natural bin j holds the value j: the
// six evaluated values are, in that order, 10, 11, 12, 4, 5, 6.  Three edges: 5, 10, 11.5 -- levels: v < 5 | 5 <= v < 10 |
// 10 <= v < 11.5 | 11.5 <= v.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scn_host.h"
#include "scn_levels.h"

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static uint32_t key_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, sizeof(b));
  return scn_trace_key(b);
}
static float float_of(uint32_t b) {
  float x;
  std::memcpy(&x, &b, sizeof(x));
  return x;
}

struct Hist {
  uint32_t cells, n_levels;
  std::vector<uint64_t> h;
  Hist(uint32_t cells_, uint32_t n_edges) : cells(cells_), n_levels(n_edges + 1), h((size_t)cells_ * (n_edges + 1), 0) {}
  bool row(uint32_t c, std::vector<uint64_t> want) const { return std::vector<uint64_t>(h.begin() + (size_t)c * n_levels, h.begin() + (size_t)(c + 1) * n_levels) == want; }
  bool empty(uint32_t c) const { return row(c, std::vector<uint64_t>(n_levels, 0)); }
  int fold(uint64_t f0, uint32_t cell_hz, const std::vector<float> &edges, const std::vector<float> &p, uint32_t units, uint32_t n, uint32_t fs,
           const std::vector<double> &fc) {
    return scn_levels_fold_spectrum(h.data(), f0, cell_hz, cells, edges.data(), (uint32_t)edges.size(), p.data(), units, n, fs, 0, 0.0, fc.data());
  }
};

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  // the first step of the search, and the level against a count by hand, for every table size: edges 0, 2, 4, ... and values on,
  // between, below and above them
  CHECK(scn_levels_top(1) == 1 && scn_levels_top(2) == 2 && scn_levels_top(3) == 2 && scn_levels_top(7) == 4 && scn_levels_top(63) == 32 &&
        scn_levels_top(128) == 128 && scn_levels_top(255) == 128);
  for (uint32_t n_edges = 1; n_edges <= SCN_LEVELS_EDGES_MAX; n_edges++) {
    std::vector<float> edges(n_edges);
    for (uint32_t e = 0; e < n_edges; e++) edges[e] = 2.0f * (float)e;
    uint32_t keys[kLevelsKeys];
    CHECK(check_levels_edges(edges.data(), n_edges, keys) == SCN_OK);
    CHECK(keys[n_edges - 1] == key_of(edges[n_edges - 1]) && keys[n_edges] == kLevelsPadKey && keys[kLevelsKeys - 1] == kLevelsPadKey);
    const uint32_t top = scn_levels_top(n_edges);
    for (int v = -1; v <= 2 * (int)n_edges; v++) {
      uint32_t want = 0;
      for (uint32_t e = 0; e < n_edges; e++) want += key_of(edges[e]) <= key_of((float)v);
      CHECK(scn_levels_level(keys, top, key_of((float)v)) == want);
    }
    CHECK(scn_levels_level(keys, top, key_of(-inf)) == 0 && scn_levels_level(keys, top, key_of(inf)) == n_edges);
    CHECK(scn_levels_level(keys, top, key_of(-0.0f)) == 0 && scn_levels_level(keys, top, key_of(0.0f)) == 1);  // (-0.0 is below the edge +0.0)
  }
  {
    // -inf and +inf as edges, -0.0 and +0.0 as two edges
    const float edges[] = {-inf, -0.0f, 0.0f, inf};
    uint32_t keys[kLevelsKeys];
    CHECK(check_levels_edges(edges, 4, keys) == SCN_OK);
    const uint32_t top = scn_levels_top(4);
    CHECK(scn_levels_level(keys, top, key_of(-inf)) == 1 && scn_levels_level(keys, top, key_of(-1.0f)) == 1 && scn_levels_level(keys, top, key_of(-0.0f)) == 2);
    CHECK(scn_levels_level(keys, top, key_of(0.0f)) == 3 && scn_levels_level(keys, top, key_of(3.0e38f)) == 3 && scn_levels_level(keys, top, key_of(inf)) == 4);
    // tables that are none: nothing written
    uint32_t untouched[kLevelsKeys];
    std::memset(untouched, 0x5a, sizeof(untouched));
    std::memcpy(keys, untouched, sizeof(keys));
    const float equal[] = {1.0f, 1.0f}, falling[] = {1.0f, 0.5f}, zeros[] = {0.0f, -0.0f}, nan_in[] = {0.0f, float_of(0x7fc00000u)}, nan_neg[] = {float_of(0xffc00001u), 0.0f};
    for (const float *bad : {equal, falling, zeros, nan_in, nan_neg}) CHECK(check_levels_edges(bad, 2, keys) == SCN_E_INVALID);
    CHECK(check_levels_edges(nullptr, 2, keys) == SCN_E_INVALID && check_levels_edges(edges, 0, keys) == SCN_E_INVALID);
    std::vector<float> many(256);
    for (uint32_t e = 0; e < 256; e++) many[e] = (float)e;
    CHECK(check_levels_edges(many.data(), 256, keys) == SCN_E_INVALID && check_levels_edges(many.data(), 255, keys) == SCN_OK);
    std::memcpy(keys, untouched, sizeof(keys));
    CHECK(check_levels_edges(equal, 2, keys) == SCN_E_INVALID && std::memcmp(keys, untouched, sizeof(keys)) == 0);
  }

  // limits
  CHECK(check_levels_geometry(1, 1, 1) == SCN_OK && check_levels_geometry(0xffffffffu, SCN_LEVELS_WORDS_MAX / 256u, 255) == SCN_OK);
  CHECK(check_levels_geometry(1, SCN_TRACE_CELLS_MAX, 3) == SCN_OK && check_levels_geometry(1, SCN_TRACE_CELLS_MAX, 4) == SCN_E_INVALID);
  CHECK(check_levels_geometry(0, 1, 1) == SCN_E_INVALID && check_levels_geometry(1, 0, 1) == SCN_E_INVALID && check_levels_geometry(1, 1, 0) == SCN_E_INVALID);
  CHECK(check_levels_geometry(1, 1, 256) == SCN_E_INVALID && check_levels_geometry(1, SCN_LEVELS_WORDS_MAX / 256u + 1u, 255) == SCN_E_INVALID);
  CHECK(check_levels_summary(4, 1000, 3) == SCN_OK && check_levels_summary(4, 1001, 0) == SCN_E_INVALID && check_levels_summary(4, 0, 4) == SCN_E_INVALID);

  // the rank: floor(permille (total - 1) / 1000), also where the product does not fit 64 bits
  CHECK(scn_levels_rank(1, 0) == 0 && scn_levels_rank(1, 1000) == 0 && scn_levels_rank(2, 500) == 0 && scn_levels_rank(2, 1000) == 1);
  CHECK(scn_levels_rank(6, 500) == 2 && scn_levels_rank(7, 500) == 3 && scn_levels_rank(1001, 1) == 1 && scn_levels_rank(1000, 1) == 0);
  CHECK(scn_levels_rank(1001, 999) == 999 && scn_levels_rank(1000, 999) == 998);
  CHECK(scn_levels_rank(~0ull, 1000) == ~0ull - 1u && scn_levels_rank(~0ull, 0) == 0);
  CHECK(scn_levels_rank(~0ull, 500) == 9223372036854775807ull);        // (2^64 - 2) / 2
  CHECK(scn_levels_rank(~0ull, 1) == 18446744073709551ull);           // floor((2^64 - 2) / 1000)
  CHECK(scn_levels_rank(~0ull, 999) == 18428297329635842062ull);      // 2^64 - 2 - ceil((2^64 - 2) / 1000) = 18446744073709551614 - 18446744073709552
  CHECK(scn_levels_rank((1ull << 63) + 1u, 500) == (1ull << 62));

  const uint32_t n = 16, fs = 8000000u;
  std::vector<float> p(n);
  for (uint32_t j = 0; j < n; j++) p[j] = (float)j;  // the bins the mask removes: 0 ... 3 (level 0), 7, 8, 9 (level 1), 13, 14, 15 (level 3)
  const std::vector<float> edges = {5.0f, 10.0f, 11.5f};
  {
    // 1 MHz cells from 97 MHz: 97.0 (10) and 97.5 (11) -> cell 0, both level 2 (10 equals an edge: the level above it);
    // 98.0 (12) -> cell 1, level 3; 102.0 (4) and 102.5 (5) -> cell 5, levels 0 and 1 (5 equals an edge); 103.0 -> cell 6 == cells
    Hist t(6, 3);
    CHECK(t.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK);
    CHECK(t.row(0, {0, 0, 2, 0}) && t.row(1, {0, 0, 0, 1}) && t.empty(2) && t.empty(3) && t.empty(4) && t.row(5, {1, 1, 0, 0}));
    // folded again: every counter doubles
    CHECK(t.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK);
    CHECK(t.row(0, {0, 0, 4, 0}) && t.row(1, {0, 0, 0, 2}) && t.empty(2) && t.row(5, {2, 2, 0, 0}));
    // a seventh cell takes 103.0 MHz (6: level 1)
    Hist t7(7, 3);
    CHECK(t7.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK && t7.row(6, {0, 1, 0, 0}) && t7.row(5, {1, 1, 0, 0}));
    // the summary of t: totals 4, 2, 0, 0, 0, 4; above level 2: 4, 2, 0, 0, 0, 0; the median's level (r = 1, 0, -, -, -, 1): 2, 3, none, 0
    uint32_t rank[6];
    uint64_t above[6], total[6];
    CHECK(scn_levels_summary(t.h.data(), 6, 4, 500, 2, rank, above, total) == SCN_OK);
    CHECK(total[0] == 4 && total[1] == 2 && total[2] == 0 && total[5] == 4 && above[0] == 4 && above[1] == 2 && above[2] == 0 && above[5] == 0);
    CHECK(rank[0] == 2 && rank[1] == 3 && rank[2] == kLevelsNoRank && rank[4] == kLevelsNoRank && rank[5] == 0);
    // cell 5 holds {2, 2, 0, 0}: permille 0 -> r 0 -> level 0; 333 -> r 0; 334 -> r 1 -> level 0; 667 -> r 2 -> level 1; 1000 -> r 3 -> level 1
    const uint32_t permilles[] = {0, 333, 334, 666, 667, 1000}, levels[] = {0, 0, 0, 0, 1, 1};
    for (int k = 0; k < 6; k++) {
      CHECK(scn_levels_summary(t.h.data(), 6, 4, permilles[k], 0, rank, nullptr, above) == SCN_OK && rank[5] == levels[k] && above[5] == 4);
    }
    CHECK(scn_levels_summary(t.h.data(), 6, 4, 500, 1, nullptr, above, nullptr) == SCN_OK && above[5] == 2 && above[0] == 4);
    CHECK(scn_levels_summary(t.h.data(), 6, 4, 500, 3, nullptr, above, nullptr) == SCN_OK && above[5] == 0 && above[0] == 0 && above[1] == 2);
  }
  {
    // all six evaluated bins in one cell: levels 0, 1, 1, 2, 2, 3 of 4, 5, 6, 10, 11, 12
    Hist t(1, 3);
    CHECK(t.fold(0, 0x80000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK && t.row(0, {1, 2, 2, 1}));
    // a centre of 1 MHz: i = 2, 3, 4 wrap to frequencies near 2^64 and fold nowhere; i = 12, 13, 14 (4, 5, 6) are 3.0, 3.5, 4.0 MHz
    Hist w(3, 3);
    CHECK(w.fold(0, 2000000u, edges, p, 1, n, fs, {1e6}) == SCN_OK && w.empty(0) && w.row(1, {1, 1, 0, 0}) && w.row(2, {0, 1, 0, 0}));
    // ... and a grid that starts at 2^64 - 2.5 MHz finds exactly them (10, 11, 12)
    Hist up(4, 3);
    CHECK(up.fold(0ull - 2500000ull, 500000u, edges, p, 1, n, fs, {1e6}) == SCN_OK);
    CHECK(up.empty(0) && up.row(1, {0, 0, 1, 0}) && up.row(2, {0, 0, 1, 0}) && up.row(3, {0, 0, 0, 1}));
  }
  {
    // special values: +-inf count (levels 0 and 3), a NaN of either sign does not, -0.0 is below the edge +0.0
    std::vector<float> q(n, 1000.0f);
    const uint32_t ev[6] = {10, 11, 12, 4, 5, 6};
    const float vals[6] = {inf, -inf, float_of(0x7fc00000u), float_of(0xffc00001u), -0.0f, 0.0f};
    for (int k = 0; k < 6; k++) q[ev[k]] = vals[k];
    Hist t(1, 3);
    CHECK(t.fold(0, 0x80000000u, {-1.0f, 0.0f, 1.0f}, q, 1, n, fs, {100e6}) == SCN_OK && t.row(0, {1, 1, 1, 1}));
    Hist none(1, 3);
    CHECK(none.fold(0, 0x80000000u, edges, std::vector<float>(n, float_of(0x7fc00000u)), 1, n, fs, {100e6}) == SCN_OK && none.empty(0));
  }
  {
    // merge: counter by counter; merge(A, B) is the histogram of everything folded into A or B; counts beyond 2^32 by doubling
    Hist a(3, 3), b(3, 3), both(3, 3);
    CHECK(a.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK);  // cells 0, 1
    CHECK(b.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {101e6}) == SCN_OK);  // 98.0, 98.5, 99.0 (10, 11, 12): cells 1, 1, 2
    CHECK(both.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {100e6}) == SCN_OK && both.fold(97000000ull, 1000000u, edges, p, 1, n, fs, {101e6}) == SCN_OK);
    CHECK(b.empty(0) && b.row(1, {0, 0, 2, 0}) && b.row(2, {0, 0, 0, 1}));
    CHECK(scn_levels_merge(a.h.data(), b.h.data(), 3, 4) == SCN_OK && a.h == both.h && a.row(1, {0, 0, 2, 1}));
    for (int k = 0; k < 61; k++) {
      const std::vector<uint64_t> copy = a.h;
      CHECK(scn_levels_merge(a.h.data(), copy.data(), 3, 4) == SCN_OK);
    }
    CHECK(a.row(0, {0, 0, 1ull << 62, 0}) && a.row(1, {0, 0, 1ull << 62, 1ull << 61}));
    uint32_t rank[3];
    uint64_t above[3], total[3];
    // cell 1: total 3 * 2^61; permille 666: r = floor(666 (3 * 2^61 - 1) / 1000) = 4607074332408960515 < 2^62 -> level 2; permille
    // 667: r = 4613991861436601597 >= 2^62 = 4611686018427387904 -> level 3
    CHECK(scn_levels_summary(a.h.data(), 3, 4, 666, 3, rank, above, total) == SCN_OK && rank[1] == 2 && above[1] == (1ull << 61) && total[1] == 3 * (1ull << 61));
    CHECK(scn_levels_rank(3 * (1ull << 61), 666) == 4607074332408960515ull && scn_levels_rank(3 * (1ull << 61), 667) == 4613991861436601597ull);
    CHECK(scn_levels_summary(a.h.data(), 3, 4, 667, 3, rank, nullptr, nullptr) == SCN_OK && rank[1] == 3 && rank[0] == 2 && rank[2] == 3);
  }
  {
    // refusals, each with nothing changed
    Hist t(4, 3);
    t.h[5] = 9;
    const std::vector<uint64_t> before = t.h;
    const std::vector<double> fc = {100e6};
    const float falling[] = {1.0f, 0.0f, 2.0f};
    uint64_t *h = t.h.data();
    CHECK(scn_levels_fold_spectrum(nullptr, 0, 1, 4, edges.data(), 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, nullptr, 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 3, nullptr, 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 3, p.data(), 1, n, fs, 0, 0.0, nullptr) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 3, nullptr, 0, n, fs, 0, 0.0, nullptr) == SCN_OK);  // (no unit: nothing to read)
    CHECK(scn_levels_fold_spectrum(h, 0, 0, 4, edges.data(), 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 0, edges.data(), 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 0, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, SCN_LEVELS_WORDS_MAX / 4u + 1u, edges.data(), 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, falling, 3, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID && std::strstr(scn_last_error(), "not above") != nullptr);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 3, p.data(), 1, 0, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_fold_spectrum(h, 0, 1, 4, edges.data(), 3, p.data(), 1, n, 0, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_levels_merge(h, nullptr, 4, 4) == SCN_E_INVALID && scn_levels_merge(nullptr, h, 4, 4) == SCN_E_INVALID && scn_levels_merge(h, h, 0, 4) == SCN_E_INVALID);
    CHECK(scn_levels_merge(h, h, 4, 1) == SCN_E_INVALID && scn_levels_merge(h, h, 4, 0) == SCN_E_INVALID && scn_levels_merge(h, h, 4, 257) == SCN_E_INVALID);
    uint32_t rank[4] = {7, 7, 7, 7};
    CHECK(scn_levels_summary(nullptr, 4, 4, 500, 0, rank, nullptr, nullptr) == SCN_E_INVALID && scn_levels_summary(h, 4, 4, 1001, 0, rank, nullptr, nullptr) == SCN_E_INVALID);
    CHECK(scn_levels_summary(h, 4, 4, 500, 4, rank, nullptr, nullptr) == SCN_E_INVALID && scn_levels_summary(h, 0, 4, 500, 0, rank, nullptr, nullptr) == SCN_E_INVALID);
    CHECK(rank[0] == 7 && rank[3] == 7 && t.h == before);
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("levels tests ok\n");
  return 0;
}
