// The trace emitters' host arithmetic (scanner_amd/csrc/scn_emitters.h: scn_emit_value, scn_emit_on, scn_emit_starts, scn_emit_peak_key,
// scn_emit_hz; scn_host.hip: check_emitters_line, scn_trace_emitters) as a stand-alone program: built by g++ -x c++ together with that
// unit, no HIP header on the include path, plain and under ASan + UBSan (tests/test_emitters_cpp.py).  Every answer is worked out by
// hand on windows of a dozen cells.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scn_emitters.h"
#include "scn_host.h"

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static_assert(sizeof(scn_emitter) == 56, "scn_emitter is 56 bytes");
static_assert(offsetof(scn_emitter, start_hz) == 0 && offsetof(scn_emitter, stop_hz) == 8 && offsetof(scn_emitter, peak_hz) == 16 &&
                  offsetof(scn_emitter, count) == 24 && offsetof(scn_emitter, first_cell) == 32 && offsetof(scn_emitter, last_cell) == 36 &&
                  offsetof(scn_emitter, peak_cell) == 40 && offsetof(scn_emitter, n_cells) == 44 && offsetof(scn_emitter, peak_db) == 48 &&
                  offsetof(scn_emitter, peak_other_db) == 52,
              "scn_emitter's fields");

static const float kInf = std::numeric_limits<float>::infinity();
static uint32_t bits_of(float x) { return scn_emit_bits(x); }

struct Window {
  std::vector<float> max_db, min_db;
  std::vector<uint64_t> count;
  explicit Window(uint32_t cells) : max_db(cells, -kInf), min_db(cells, kInf), count(cells, 0) {}
  void set(uint32_t c, float mx, float mn, uint64_t k) { max_db[c] = mx, min_db[c] = mn, count[c] = k; }
  // the whole list; *status the call's
  std::vector<scn_emitter> list(uint32_t line, float thr, uint32_t gap, uint64_t f0 = 1000, uint32_t hz = 10, uint32_t first_cell = 0, int *status = nullptr) {
    uint64_t total = 99;
    int st = scn_trace_emitters(max_db.data(), min_db.data(), count.data(), f0, hz, (uint32_t)count.size(), first_cell, line, thr, gap, nullptr, 0, &total);
    CHECK(st == (total ? SCN_E_TRUNCATED : SCN_OK));
    std::vector<scn_emitter> out(total);
    st = scn_trace_emitters(max_db.data(), min_db.data(), count.data(), f0, hz, (uint32_t)count.size(), first_cell, line, thr, gap, out.data(), out.size(),
                            &total);
    CHECK(total == out.size());
    if (status) *status = st;
    else CHECK(st == SCN_OK);
    return out;
  }
};

static bool is(const scn_emitter &r, uint32_t first, uint32_t last, uint32_t peak, uint32_t n, uint64_t count, float peak_db, float other) {
  return r.first_cell == first && r.last_cell == last && r.peak_cell == peak && r.n_cells == n && r.count == count && bits_of(r.peak_db) == bits_of(peak_db) &&
         bits_of(r.peak_other_db) == bits_of(other);
}

static void test_arithmetic() {
  // the value of a line
  CHECK(scn_emit_value(kEmitLineMax, bits_of(3.0f), bits_of(1.0f)) == bits_of(3.0f));
  CHECK(scn_emit_value(kEmitLineMin, bits_of(3.0f), bits_of(1.0f)) == bits_of(1.0f));
  CHECK(scn_emit_value(kEmitLineSpread, bits_of(3.0f), bits_of(1.0f)) == bits_of(2.0f));
  CHECK(scn_emit_value(kEmitLineSpread, 0x00c00000u, 0x00800000u) == 0x00400000u);  // 1.5 * 2^-126 - 2^-126 = 2^-127, a denormal, kept
  CHECK(scn_trace_is_nan(scn_emit_value(kEmitLineSpread, bits_of(kInf), bits_of(kInf))));
  CHECK(scn_trace_is_nan(scn_emit_value(kEmitLineSpread, bits_of(-kInf), bits_of(-kInf))));
  CHECK(scn_emit_value(kEmitLineSpread, bits_of(kInf), bits_of(-kInf)) == bits_of(kInf));
  CHECK(scn_emit_other(kEmitLineMax, 1u, 2u) == 2u && scn_emit_other(kEmitLineMin, 1u, 2u) == 1u && scn_emit_other(kEmitLineSpread, 1u, 2u) == 1u);
  // on: strict, a NaN never, -0.0 equal to +0.0, an empty cell never
  CHECK(scn_emit_on(1, bits_of(1.0f), bits_of(0.5f)) && !scn_emit_on(1, bits_of(1.0f), bits_of(1.0f)) && !scn_emit_on(0, bits_of(1.0f), bits_of(0.5f)));
  CHECK(!scn_emit_on(1, bits_of(0.0f), bits_of(-0.0f)) && !scn_emit_on(1, bits_of(-0.0f), bits_of(0.0f)) && !scn_emit_on(1, bits_of(-0.0f), bits_of(-0.0f)));
  CHECK(scn_emit_on(1, 0x00000001u, bits_of(0.0f)) && scn_emit_on(1, 0x00000001u, bits_of(-0.0f)) && !scn_emit_on(1, 0x80000001u, bits_of(-0.0f)));
  CHECK(scn_emit_on(1, bits_of(0.0f), 0x80000001u) && scn_emit_on(1, bits_of(-0.0f), 0x80000001u));
  CHECK(!scn_emit_on(1, 0x7fc00000u, bits_of(-kInf)) && !scn_emit_on(1, 0xffc00001u, bits_of(-kInf)));
  CHECK(!scn_emit_on(1, bits_of(-kInf), bits_of(-kInf)) && scn_emit_on(1, bits_of(-3.0e38f), bits_of(-kInf)) && !scn_emit_on(1, bits_of(kInf), bits_of(kInf)));
  CHECK(scn_emit_on(1, bits_of(kInf), bits_of(3.0e38f)) && scn_emit_on(1ull << 40, bits_of(-1.0f), bits_of(-1.0000001f)));
  // starts: the first on cell, or more than max_gap + 1 beyond the previous one
  CHECK(scn_emit_starts(false, 0, 0, 0xffffffffu) && !scn_emit_starts(true, 4, 5, 0) && scn_emit_starts(true, 4, 6, 0) && !scn_emit_starts(true, 4, 6, 1));
  CHECK(!scn_emit_starts(true, 0, 0xffffffffu, 0xfffffffeu) && scn_emit_starts(true, 0, 0xffffffffu, 0xfffffffdu) && !scn_emit_starts(true, 0, 0xffffffffu, 0xffffffffu));
  // the peak key: the larger value, then the lower cell; -0.0 below +0.0; never 0
  CHECK(scn_emit_peak_key(bits_of(2.0f), 9) > scn_emit_peak_key(bits_of(1.0f), 3) && scn_emit_peak_key(bits_of(1.0f), 3) > scn_emit_peak_key(bits_of(1.0f), 4));
  CHECK(scn_emit_peak_key(bits_of(0.0f), 9) > scn_emit_peak_key(bits_of(-0.0f), 3) && scn_emit_peak_key(bits_of(-kInf), 0xffffffffu) != 0);
  CHECK(scn_emit_peak_cell(scn_emit_peak_key(bits_of(-7.5f), 123456)) == 123456 && scn_emit_peak_bits(scn_emit_peak_key(bits_of(-7.5f), 123456)) == bits_of(-7.5f));
  CHECK(scn_emit_peak_bits(scn_emit_peak_key(0x80000000u, 0)) == 0x80000000u && scn_emit_peak_cell(scn_emit_peak_key(0u, 0)) == 0);
  // hertz: uint64, wrapping
  CHECK(scn_emit_hz(1000, 10, 7) == 1070 && scn_emit_hz(0xffffffffffffffffull, 0xffffffffu, 1) == 0xfffffffeull);
  CHECK(scn_emit_hz(5, 0xffffffffu, 1ull << 22) == 5 + 0xffffffffull * (1ull << 22));
}

static void test_runs() {
  Window w(12);
  //   cell     0    1    2    3    4    5    6    7    8    9   10   11
  //   max     -5   -1   -2    e   -1   -9   -1   -1   -5    e    e   -3        threshold -4 on MAX: on = 1 2 4 6 7 11
  w.set(0, -5, -8, 3), w.set(1, -1, -6, 2), w.set(2, -2, -7, 5), w.set(4, -1, -9, 1), w.set(5, -9, -9, 1), w.set(6, -1, -3, 4), w.set(7, -1, -2, 8), w.set(8, -5, -6, 2);
  w.set(11, -3, -3, 1);
  std::vector<scn_emitter> r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 0);
  CHECK(r.size() == 4);
  if (r.size() == 4) {
    CHECK(is(r[0], 1, 2, 1, 2, 7, -1.0f, -6.0f) && r[0].start_hz == 1010 && r[0].stop_hz == 1030 && r[0].peak_hz == 1010);
    CHECK(is(r[1], 4, 4, 4, 1, 1, -1.0f, -9.0f) && r[1].start_hz == 1040 && r[1].stop_hz == 1050);
    CHECK(is(r[2], 6, 7, 6, 2, 12, -1.0f, -3.0f));  // equal peaks: the lowest cell
    CHECK(is(r[3], 11, 11, 11, 1, 1, -3.0f, -3.0f) && r[3].stop_hz == 1120);
  }
  r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 1);  // bridges cell 3 (empty) and cell 5 (quiet), not 8 ... 10
  CHECK(r.size() == 2);
  if (r.size() == 2) CHECK(is(r[0], 1, 7, 1, 5, 20, -1.0f, -6.0f) && is(r[1], 11, 11, 11, 1, 1, -3.0f, -3.0f));
  r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 2);  // 7 -> 11 needs max_gap 3
  CHECK(r.size() == 2);
  r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 3);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 1, 11, 1, 6, 21, -1.0f, -6.0f));
  r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 0xffffffffu);
  CHECK(r.size() == 1);
  // the threshold equal to a value: off; -inf: every non-empty cell
  r = w.list(SCN_TRACE_LINE_MAX, -1.0f, 0);
  CHECK(r.empty());
  r = w.list(SCN_TRACE_LINE_MAX, -kInf, 0);
  CHECK(r.size() == 3);
  if (r.size() == 3) CHECK(is(r[0], 0, 2, 1, 3, 10, -1.0f, -6.0f) && is(r[1], 4, 8, 4, 5, 16, -1.0f, -9.0f) && is(r[2], 11, 11, 11, 1, 1, -3.0f, -3.0f));
  r = w.list(SCN_TRACE_LINE_MAX, kInf, 0);
  CHECK(r.empty());
  // MIN: peak_other is the cell's max; threshold -6.5: on = 1 6 7 8 11
  r = w.list(SCN_TRACE_LINE_MIN, -6.5f, 0);
  CHECK(r.size() == 3);
  if (r.size() == 3) CHECK(is(r[0], 1, 1, 1, 1, 2, -6.0f, -1.0f) && is(r[1], 6, 8, 7, 3, 14, -2.0f, -1.0f) && is(r[2], 11, 11, 11, 1, 1, -3.0f, -3.0f));
  // SPREAD: 3 5 5 e 8 0 2 1 1 e e 0; above 1.5: 0 1 2 4 6; the count-1 cells read 0.0 and are off at threshold 0
  r = w.list(SCN_TRACE_LINE_SPREAD, 1.5f, 0);
  CHECK(r.size() == 3);
  if (r.size() == 3) CHECK(is(r[0], 0, 2, 1, 3, 10, 5.0f, -1.0f) && is(r[1], 4, 4, 4, 1, 1, 8.0f, -1.0f) && is(r[2], 6, 6, 6, 1, 4, 2.0f, -1.0f));
  r = w.list(SCN_TRACE_LINE_SPREAD, 0.0f, 0);
  CHECK(r.size() == 3);  // cell 5 (0.0) still cuts 4 from 6 ... 8
  if (r.size() == 3) CHECK(is(r[0], 0, 2, 1, 3, 10, 5.0f, -1.0f) && is(r[1], 4, 4, 4, 1, 1, 8.0f, -1.0f) && is(r[2], 6, 8, 6, 3, 14, 2.0f, -1.0f));
  r = w.list(SCN_TRACE_LINE_SPREAD, 0.0f, 1);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 0, 8, 4, 7, 25, 8.0f, -1.0f));
  // a window in the middle of a trace: absolute cells, hertz from the trace's cell 0; f0 + cell * cell_hz wraps in uint64
  r = w.list(SCN_TRACE_LINE_MAX, -4.0f, 0, 0xfffffffffffffff0ull, 4, 100);
  CHECK(r.size() == 4);
  if (r.size() == 4) CHECK(is(r[0], 101, 102, 101, 2, 7, -1.0f, -6.0f) && r[0].start_hz == 0xfffffffffffffff0ull + 404 && r[0].stop_hz == 0xfffffffffffffff0ull + 412);
}

static void test_values() {
  Window w(8);
  w.set(0, kInf, kInf, 1);            // spread: NaN, off
  w.set(1, -kInf, -kInf, 2);          // max -inf: on at no threshold; spread: NaN
  w.set(2, 0.0f, -0.0f, 1ull << 40);  // spread 0.0
  w.set(3, -0.0f, -0.0f, 1ull << 40);
  w.set(4, scn_emit_float(0x00c00000u), scn_emit_float(0x00800000u), 1ull << 40);  // spread 2^-127
  w.set(5, kInf, -kInf, 1);           // spread +inf
  w.set(7, 1.0f, 1.0f, 0);            // count 0: empty whatever it holds
  std::vector<scn_emitter> r = w.list(SCN_TRACE_LINE_SPREAD, 0.0f, 0);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 4, 5, 5, 2, (1ull << 40) + 1, kInf, kInf));
  r = w.list(SCN_TRACE_LINE_SPREAD, -kInf, 0);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 2, 5, 5, 4, 3 * (1ull << 40) + 1, kInf, kInf));
  r = w.list(SCN_TRACE_LINE_MAX, -kInf, 0);  // cell 1 (-inf) is off; +0.0 beats -0.0 and the denormal beats both; +inf twice: the lowest cell
  CHECK(r.size() == 2);
  if (r.size() == 2) CHECK(is(r[0], 0, 0, 0, 1, 1, kInf, kInf) && is(r[1], 2, 5, 5, 4, 3 * (1ull << 40) + 1, kInf, -kInf));
  r = w.list(SCN_TRACE_LINE_MAX, -1.0f, 0, 0, 1, 2);
  CHECK(r.size() == 2);
  Window z(3);
  z.set(0, -0.0f, -0.0f, 1), z.set(1, 0.0f, -0.0f, 1), z.set(2, 0.0f, 0.0f, 1);
  r = z.list(SCN_TRACE_LINE_MAX, -1.0f, 0);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 0, 2, 1, 3, 3, 0.0f, -0.0f));
  r = z.list(SCN_TRACE_LINE_MIN, -1.0f, 0);
  if (r.size() == 1) CHECK(is(r[0], 0, 2, 2, 3, 3, 0.0f, 0.0f));
  else CHECK(false);
}

static void test_refusals() {
  Window w(4);
  w.set(0, 1, 1, 1), w.set(2, 1, 1, 1), w.set(3, 1, 1, 1);
  uint64_t total = 7;
  scn_emitter out[4];
  std::memset(out, 0xab, sizeof(out));
  float *mx = w.max_db.data(), *mn = w.min_db.data();
  uint64_t *ct = w.count.data();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, out, 4, &total) == SCN_OK && total == 2);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, out, 1, &total) == SCN_E_TRUNCATED && total == 2 && out[0].first_cell == 0 && out[0].n_cells == 1);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, nullptr, 0, &total) == SCN_E_TRUNCATED && total == 2);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 5.0f, 0, nullptr, 0, &total) == SCN_OK && total == 0);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, nullptr, 1, &total) == SCN_E_INVALID && total == 0);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, out, 4, nullptr) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(nullptr, mn, ct, 0, 1, 4, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, nullptr, ct, 0, 1, 4, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, nullptr, 0, 1, 4, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 0, 4, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 0, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, SCN_TRACE_CELLS_MAX + 1u, 0, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, SCN_TRACE_CELLS_MAX - 3u, 0, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, SCN_TRACE_CELLS_MAX - 4u, 0, 0.0f, 0, out, 4, &total) == SCN_OK && out[1].last_cell == SCN_TRACE_CELLS_MAX - 1u);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 3, 0.0f, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, nan, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(scn_trace_emitters(mx, mn, ct, 0, 1, 4, 0, 0, -nan, 0, out, 4, &total) == SCN_E_INVALID);
  CHECK(check_emitters_line(2, -kInf) == SCN_OK && check_emitters_line(0, kInf) == SCN_OK && check_emitters_line(3, 0.0f) == SCN_E_INVALID);
}

// the largest window, every other cell on: cells / 2 records, and one record at max_gap 1
static void test_largest() {
  const uint32_t cells = SCN_TRACE_CELLS_MAX;
  Window w(cells);
  for (uint32_t c = 0; c < cells; c += 2) w.set(c, (float)(c % 1000u), -1.0f, 1ull << 40);
  std::vector<scn_emitter> r = w.list(SCN_TRACE_LINE_MAX, -0.5f, 0, 0, 0xffffffffu);
  CHECK(r.size() == cells / 2);
  if (r.size() == cells / 2) {
    const scn_emitter &l = r.back();
    CHECK(is(l, cells - 2, cells - 2, cells - 2, 1, 1ull << 40, (float)((cells - 2) % 1000u), -1.0f) && l.stop_hz == (uint64_t)(cells - 1) * 0xffffffffull);
  }
  r = w.list(SCN_TRACE_LINE_MAX, -0.5f, 1);
  CHECK(r.size() == 1);
  if (r.size() == 1) CHECK(is(r[0], 0, cells - 2, 998, cells / 2, (uint64_t)(cells / 2) << 40, 998.0f, -1.0f));
}

int main() {
  test_arithmetic();
  test_runs();
  test_values();
  test_refusals();
  test_largest();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("emitters tests ok\n");
  return 0;
}
