// The sweep trace's host arithmetic (scanner_amd/csrc/scn_trace.h: scn_trace_key, scn_trace_unkey, scn_trace_is_nan, scn_trace_freq,
// scn_trace_cell; scn_host.hip: check_trace_geometry, check_trace_range, scn_trace_init, scn_trace_fold_spectrum, scn_trace_merge) as
// a stand-alone program: built by g++ -x c++ together with that unit, no HIP header on the include path, plain and under ASan + UBSan
// (tests/test_trace_cpp.py).  Known answers worked out by hand for n = 16 at 8 MHz with the default mask: the evaluated fftshift
// indices are i in {2, 3, 4, 12, 13, 14} (natural bins j = 10, 11, 12, 4, 5, 6), bin_step = 500000, and a unit centred at 100 MHz has
// start_frequency 96 MHz: its evaluated bins lie at 97.0, 97.5, 98.0, 102.0, 102.5 and 103.0 MHz.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scn_host.h"
#include "scn_trace.h"

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static uint32_t bits_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}
static float float_of(uint32_t b) {
  float x;
  std::memcpy(&x, &b, sizeof(x));
  return x;
}

struct Trace {
  std::vector<float> max_db, min_db;
  std::vector<uint64_t> count;
  explicit Trace(uint32_t cells) : max_db(cells, 123.0f), min_db(cells, 123.0f), count(cells, 77) {
    CHECK(scn_trace_init(max_db.data(), min_db.data(), count.data(), cells) == SCN_OK);
  }
  bool empty(uint32_t c) const { return bits_of(max_db[c]) == 0xff800000u && bits_of(min_db[c]) == 0x7f800000u && count[c] == 0; }
  bool holds(uint32_t c, float mx, float mn, uint64_t k) const {
    return bits_of(max_db[c]) == bits_of(mx) && bits_of(min_db[c]) == bits_of(mn) && count[c] == k;
  }
  int fold(uint64_t f0, uint32_t cell_hz, const std::vector<float> &p, uint32_t units, uint32_t n, uint32_t fs, const std::vector<double> &fc) {
    return scn_trace_fold_spectrum(max_db.data(), min_db.data(), count.data(), f0, cell_hz, (uint32_t)count.size(), p.data(), units, n, fs, 0, 0.0,
                                   fc.data());
  }
};

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  // the key: unsigned order = float order, -inf lowest, -0.0 below +0.0; its inverse; what is a NaN
  const float ordered[] = {-inf, -3.0e38f, -1.0f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1.0f, 3.0e38f, inf};
  for (size_t k = 0; k + 1 < sizeof(ordered) / sizeof(ordered[0]); k++) CHECK(scn_trace_key(bits_of(ordered[k])) < scn_trace_key(bits_of(ordered[k + 1])));
  for (float x : ordered) CHECK(scn_trace_unkey(scn_trace_key(bits_of(x))) == bits_of(x) && !scn_trace_is_nan(bits_of(x)));
  CHECK(scn_trace_key(0xff800000u) == kTraceEmptyMaxKey && scn_trace_key(0x7f800000u) == kTraceEmptyMinKey);
  CHECK(scn_trace_is_nan(0x7fc00000u) && scn_trace_is_nan(0xffc00001u) && scn_trace_is_nan(0x7f800001u) && scn_trace_is_nan(0xffffffffu));

  // the frequency of a bin: the double addition, the uint32 product, the x86 cast
  CHECK(scn_trace_start(100e6, 8000000u) == 96e6 && scn_trace_start(100e6, 8000001u) == 96e6);  // (uint32 division)
  CHECK(scn_trace_freq(96e6, 2, 500000u) == 97000000ull && scn_trace_freq(96e6 + 0.75, 2, 500000u) == 97000000ull);
  CHECK(scn_trace_freq(-3e6, 2, 500000u) == 0ull - 2000000ull && scn_trace_freq(-3e6, 6, 500000u) == 0ull && scn_trace_freq(-0.5, 0, 1u) == 0ull);
  CHECK(scn_trace_freq(0.0, 3, 0x80000000u) == 0x80000000ull && scn_trace_freq(0.0, 2, 0x80000000u) == 0ull);  // i * bin_step wraps in uint32
  // the cell: uint64 integer arithmetic, below the grid and at or beyond its end skipped, both division widths
  CHECK(scn_trace_cell(97000000ull, 97000000ull, 1000000u, 6) == 0 && scn_trace_cell(96999999ull, 97000000ull, 1000000u, 6) == kTraceNoCell);
  CHECK(scn_trace_cell(102999999ull, 97000000ull, 1000000u, 6) == 5 && scn_trace_cell(103000000ull, 97000000ull, 1000000u, 6) == kTraceNoCell);
  CHECK(scn_trace_cell(4300000000ull, 0, 2000u, 1u << 22) == 2150000u && scn_trace_cell(1ull << 40, 0, 3u, 1u << 22) == kTraceNoCell);
  CHECK(scn_trace_cell(0ull - 2000000ull, 0, 0xffffffffu, 1u << 22) == kTraceNoCell);  // (a wrapped frequency: 2^64 / 2^32 cells away)
  CHECK(scn_trace_cell(0ull - 2000000ull, 0ull - 2500000ull, 500000u, 4) == 1u);
  CHECK(scn_trace_cell(0xffffffffull, 0, 1u, 1u << 22) == kTraceNoCell && scn_trace_cell((1ull << 32) + 5u, 1ull << 32, 1u, 8) == 5u);

  // a unit's cells from integers alone (scn_trace_unit) are the cells of scn_trace_freq + scn_trace_cell, wherever it says `exact`
  {
    const double starts[] = {0.0, 1.0, 96e6, 96000000.5, -3e6, -0.0, 4503599627370495.0, 4503599627370496.0, 1e19, 49e9, 4294967296.0};
    const uint64_t f0s[] = {0, 1, 95999999ull, 96000000ull, 96000001ull, 4294967296ull, 1ull << 40, 0ull - 3000000ull};
    const uint32_t cell_hzs[] = {1u, 7u, 1953u, 124992u, 0x80000000u, 0xffffffffu};
    const uint32_t ks[] = {0u, 1u, 1952u, 1953u, 500000u, 7998000u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    uint32_t exact = 0;
    for (double start : starts)
      for (uint64_t f0 : f0s)
        for (uint32_t cell_hz : cell_hzs) {
          const ScnTraceUnit u = scn_trace_unit(start, f0, cell_hz);
          CHECK(u.exact == (start >= 0.0 && start < 4503599627370496.0 && start == std::floor(start) && (uint64_t)start >= f0));
          if (!u.exact) continue;
          exact++;
          for (uint32_t k : ks)
            for (uint32_t cells : {1u, 6u, 1u << 22}) {
              // (scn_trace_freq with i = k, bin_step = 1: the same uint32 offset)
              CHECK(scn_trace_cell_in_unit(u, k, cell_hz, cells) == scn_trace_cell(scn_trace_freq(start, k, 1u), f0, cell_hz, cells));
            }
        }
    CHECK(exact >= 100);
    CHECK(!scn_trace_unit(96000000.5, 0, 1).exact && !scn_trace_unit(-3e6, 0, 1).exact && !scn_trace_unit(96e6, 96000001ull, 1).exact);
    CHECK(!scn_trace_unit(std::numeric_limits<double>::quiet_NaN(), 0, 1).exact && scn_trace_unit(96e6, 96000000ull, 1).exact);
  }

  // limits
  CHECK(check_trace_geometry(1, 1) == SCN_OK && check_trace_geometry(0xffffffffu, SCN_TRACE_CELLS_MAX) == SCN_OK);
  CHECK(check_trace_geometry(0, 1) == SCN_E_INVALID && check_trace_geometry(1, 0) == SCN_E_INVALID && check_trace_geometry(1, SCN_TRACE_CELLS_MAX + 1u) == SCN_E_INVALID);
  CHECK(check_trace_range(8, 0, 8) == SCN_OK && check_trace_range(8, 8, 0) == SCN_OK && check_trace_range(0, 0, 0) == SCN_OK);
  CHECK(check_trace_range(8, 1, 8) == SCN_E_INVALID && check_trace_range(8, 0xffffffffu, 2) == SCN_E_INVALID && check_trace_range(0, 0, 1) == SCN_E_INVALID);

  // one unit at 100 MHz; natural bin j holds the value j, the bins the mask removes 1000 + j (they would win every maximum)
  const uint32_t n = 16, fs = 8000000u;
  std::vector<float> p(n);
  for (uint32_t j = 0; j < n; j++) p[j] = (j >= 4 && j <= 6) || (j >= 10 && j <= 12) ? (float)j : 1000.0f + (float)j;
  {
    // 1 MHz cells from 97 MHz: 97.0 and 97.5 -> cell 0, 98.0 -> 1, 102.0 and 102.5 -> 5, 103.0 -> 6 == cells: skipped
    Trace t(6);
    for (uint32_t c = 0; c < 6; c++) CHECK(t.empty(c));
    CHECK(t.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6}) == SCN_OK);
    CHECK(t.holds(0, 11.0f, 10.0f, 2) && t.holds(1, 12.0f, 12.0f, 1) && t.empty(2) && t.empty(3) && t.empty(4) && t.holds(5, 5.0f, 4.0f, 2));
    // folded again: counts twice, maximum and minimum stay
    CHECK(t.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6}) == SCN_OK);
    CHECK(t.holds(0, 11.0f, 10.0f, 4) && t.holds(1, 12.0f, 12.0f, 2) && t.empty(2) && t.holds(5, 5.0f, 4.0f, 4));
    // a seventh cell takes 103.0 MHz
    Trace t7(7);
    CHECK(t7.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6}) == SCN_OK && t7.holds(6, 6.0f, 6.0f, 1) && t7.holds(5, 5.0f, 4.0f, 2));
  }
  {
    // f0 one hertz above 97.5 MHz, cells of one bin_step: 97.0 and 97.5 lie below the grid; 98.0 -> (499999) / 500000 = 0,
    // 102.0 -> 8, 102.5 -> 9, 103.0 -> 10 == cells: skipped
    Trace t(10);
    CHECK(t.fold(97500001ull, 500000u, p, 1, n, fs, {100e6}) == SCN_OK);
    CHECK(t.holds(0, 12.0f, 12.0f, 1) && t.holds(8, 4.0f, 4.0f, 1) && t.holds(9, 5.0f, 5.0f, 1));
    for (uint32_t c = 1; c < 8; c++) CHECK(t.empty(c));
  }
  {
    // a centre with a fraction: 96000000.75 + 1000000 -> 97000000 (truncated), the same cells as without it
    Trace t(6);
    CHECK(t.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6 + 0.75}) == SCN_OK && t.holds(0, 11.0f, 10.0f, 2) && t.holds(5, 5.0f, 4.0f, 2));
  }
  {
    // a centre of 1 MHz: start_frequency -3 MHz.  i = 2, 3, 4 are -2.0, -1.5, -1.0 MHz and wrap to 2^64 minus that; i = 12, 13, 14
    // are 3.0, 3.5, 4.0 MHz.  From 0 Hz in 2 MHz cells: cell 1 twice, cell 2 once, and the wrapped bins nowhere
    Trace t(3);
    CHECK(t.fold(0, 2000000u, p, 1, n, fs, {1e6}) == SCN_OK && t.empty(0) && t.holds(1, 5.0f, 4.0f, 2) && t.holds(2, 6.0f, 6.0f, 1));
    // ... and a grid that starts at 2^64 - 2.5 MHz finds exactly them: the cast is the two's complement
    Trace w(4);
    CHECK(w.fold(0ull - 2500000ull, 500000u, p, 1, n, fs, {1e6}) == SCN_OK);
    CHECK(w.empty(0) && w.holds(1, 10.0f, 10.0f, 1) && w.holds(2, 11.0f, 11.0f, 1) && w.holds(3, 12.0f, 12.0f, 1));
  }
  {
    // sample_rate < n: bin_step 0, the whole unit at fc - sample_rate / 2 = 995 Hz
    Trace t(2);
    CHECK(t.fold(990, 10u, p, 1, n, 10u, {1000.0}) == SCN_OK && t.holds(0, 12.0f, 4.0f, 6) && t.empty(1));
  }
  {
    // special values in one cell: -0.0 below +0.0, +-inf fold, a NaN of either sign does not; two units on one centre
    std::vector<float> q(2 * n, 1000.0f);
    const uint32_t ev[6] = {10, 11, 12, 4, 5, 6};
    const float first[6] = {-0.0f, 0.0f, float_of(0x7fc00000u), -0.0f, float_of(0xffc00001u), 0.0f};
    const float second[6] = {inf, -inf, 1.0f, float_of(0x7fc00000u), 2.0f, 3.0f};
    for (int k = 0; k < 6; k++) q[ev[k]] = first[k], q[n + ev[k]] = second[k];
    Trace t(1);
    CHECK(t.fold(0, 0x80000000u, q, 1, n, fs, {100e6}) == SCN_OK && t.holds(0, 0.0f, -0.0f, 4));
    CHECK(t.fold(0, 0x80000000u, std::vector<float>(q.begin() + n, q.end()), 1, n, fs, {100e6}) == SCN_OK && t.holds(0, inf, -inf, 9));
    Trace both(1);
    CHECK(both.fold(0, 0x80000000u, q, 2, n, fs, {100e6, 100e6}) == SCN_OK && both.holds(0, inf, -inf, 9));
    // a unit that is all NaN changes nothing
    Trace none(1);
    CHECK(none.fold(0, 0x80000000u, std::vector<float>(n, float_of(0x7fc00000u)), 1, n, fs, {100e6}) == SCN_OK && none.empty(0));
  }
  {
    // merge: counts added, the larger maximum and the smaller minimum by key; an empty cell is the neutral element
    Trace a(3), b(3), both(3);
    CHECK(a.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6}) == SCN_OK);  // cells 0, 1 (and 5, outside)
    CHECK(b.fold(97000000ull, 1000000u, p, 1, n, fs, {101e6}) == SCN_OK);  // 98.0, 98.5, 99.0: cells 1, 1, 2
    CHECK(both.fold(97000000ull, 1000000u, p, 1, n, fs, {100e6}) == SCN_OK && both.fold(97000000ull, 1000000u, p, 1, n, fs, {101e6}) == SCN_OK);
    CHECK(b.empty(0) && b.holds(1, 11.0f, 10.0f, 2) && b.holds(2, 12.0f, 12.0f, 1));
    CHECK(scn_trace_merge(a.max_db.data(), a.min_db.data(), a.count.data(), b.max_db.data(), b.min_db.data(), b.count.data(), 3) == SCN_OK);
    CHECK(a.holds(0, 11.0f, 10.0f, 2) && a.holds(1, 12.0f, 10.0f, 3) && a.holds(2, 12.0f, 12.0f, 1));
    CHECK(a.max_db == both.max_db && a.min_db == both.min_db && a.count == both.count);
  }
  {
    // refusals, each with nothing changed
    Trace t(4);
    const std::vector<double> fc = {100e6};
    float *mx = t.max_db.data(), *mn = t.min_db.data();
    uint64_t *ct = t.count.data();
    CHECK(scn_trace_fold_spectrum(nullptr, mn, ct, 0, 1, 4, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, nullptr, ct, 0, 1, 4, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, nullptr, 0, 1, 4, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 4, nullptr, 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 4, p.data(), 1, n, fs, 0, 0.0, nullptr) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 4, nullptr, 0, n, fs, 0, 0.0, nullptr) == SCN_OK);  // (no unit: nothing to read)
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 0, 4, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID && std::strstr(scn_last_error(), "1 Hz") != nullptr);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 0, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, SCN_TRACE_CELLS_MAX + 1u, p.data(), 1, n, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 4, p.data(), 1, 0, fs, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_fold_spectrum(mx, mn, ct, 0, 1, 4, p.data(), 1, n, 0, 0, 0.0, fc.data()) == SCN_E_INVALID);
    CHECK(scn_trace_init(mx, mn, ct, 0) == SCN_E_INVALID && scn_trace_init(nullptr, mn, ct, 4) == SCN_E_INVALID);
    CHECK(scn_trace_merge(mx, mn, ct, mx, mn, nullptr, 4) == SCN_E_INVALID && scn_trace_merge(mx, mn, ct, mx, mn, ct, 0) == SCN_E_INVALID);
    for (uint32_t c = 0; c < 4; c++) CHECK(t.empty(c));
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("trace tests ok\n");
  return 0;
}
