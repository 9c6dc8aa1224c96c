// The floor window's host arithmetic (scanner_amd/csrc/scn_host.hip: floor_window_ranks, scn_local_floor_from_spectrum) as a
// stand-alone program: built by g++ -x c++ together with that unit, no HIP header on the include path, plain and under ASan + UBSan
// (tests/test_local_floor_cpp.py).  The edge sizes: windows that reach past both band edges, over the DC hole and over the whole
// spectrum, odd n, the largest window, and the rejections -- against a sort of each bin's cells written out here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scn_host.h"

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, sizeof(b));
  return b;
}
static uint32_t key_of(float f) {
  const uint32_t b = bits_of(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct Mask {
  uint32_t dc_ignore, i_lo, i_hi;
};

// a spectrum with ties, both zeros, -inf and +inf among ordinary values (a fixed recurrence: no library generator)
static std::vector<float> spectrum(uint32_t n, uint32_t seed) {
  std::vector<float> s(n);
  uint32_t x = seed * 2654435761u + 12345u;
  for (uint32_t j = 0; j < n; j++) {
    x = x * 1664525u + 1013904223u;
    const uint32_t pick = (x >> 8) % 16u;
    const float v = (float)((int)((x >> 12) % 2001u) - 1000) * 0.03125f;
    s[j] = pick == 0 ? -std::numeric_limits<float>::infinity() : pick == 1 ? 0.0f : pick == 2 ? -0.0f : pick == 3 ? 7.5f
           : pick == 4 ? std::numeric_limits<float>::infinity() : v;
  }
  return s;
}

// the definition, bin by bin: gather the evaluated bins guard < |i' - i| <= guard + train inside [0, n), sort their keys, take the rank
static bool brute(const std::vector<float> &s, const Mask &m, uint32_t permille, uint32_t train, uint32_t guard, std::vector<float> &out,
                  std::vector<uint32_t> &cells_of) {
  const uint32_t n = (uint32_t)s.size();
  cells_of.assign(n, 0);
  bool every_bin_has_a_cell = true;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = (i + n / 2) % n;
    if (!scn_bin_evaluated(j, i, n, m)) continue;
    std::vector<uint32_t> keys;
    for (uint32_t c = 0; c < n; c++) {
      const uint32_t d = c > i ? c - i : i - c, jc = (c + n / 2) % n;
      if (d > guard && d <= guard + train && scn_bin_evaluated(jc, c, n, m)) keys.push_back(key_of(s[jc]));
    }
    cells_of[i] = (uint32_t)keys.size();
    if (keys.empty()) {
      every_bin_has_a_cell = false;
      continue;
    }
    std::sort(keys.begin(), keys.end());
    const uint32_t key = keys[(size_t)((uint64_t)permille * (keys.size() - 1u) / 1000u)];
    const uint32_t b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    std::memcpy(&out[j], &b, sizeof(b));
  }
  return every_bin_has_a_cell;
}

static void check_case(uint32_t n, uint32_t dc_arg, double ub_arg, uint32_t permille_arg, uint32_t train, uint32_t guard) {
  const std::vector<float> s = spectrum(n, n + train);
  Mask m = {dc_arg == 0 ? 4u : dc_arg == SCN_DC_IGNORE_NONE ? 0u : dc_arg, 0, 0};
  const uint32_t kept = evaluated_bins(n, m.dc_ignore, ub_arg == 0.0 ? 0.75 : ub_arg, &m.i_lo, &m.i_hi);
  uint32_t permille = 0;
  CHECK(floor_permille_of(permille_arg, &permille));
  const float sentinel = -4321.25f;
  std::vector<float> want(n, sentinel), got(n, sentinel);
  std::vector<uint32_t> cells_of;
  const bool ok = kept != 0 && brute(s, m, permille, train, guard, want, cells_of);
  const int st = scn_local_floor_from_spectrum(s.data(), n, dc_arg, ub_arg, permille_arg, train, guard, got.data());
  CHECK((st == SCN_OK) == ok);
  if (st != SCN_OK) {
    CHECK(st == SCN_E_INVALID);
    for (uint32_t j = 0; j < n; j++) CHECK(bits_of(got[j]) == bits_of(sentinel));  // nothing written
    return;
  }
  for (uint32_t j = 0; j < n; j++) CHECK(bits_of(got[j]) == bits_of(want[j]));  // the floors, and the sentinel where the mask removes the bin
  // the table the GPU's kernel reads: r_i + 1 by fftshift index, 0 where the mask removes the bin
  std::vector<uint16_t> need;
  CHECK(floor_window_ranks(n, m.dc_ignore, m.i_lo, m.i_hi, permille, train, guard, need) == SCN_OK);
  CHECK(need.size() == n);
  for (uint32_t i = 0; i < n && need.size() == n; i++) {
    const bool ev = scn_bin_evaluated((i + n / 2) % n, i, n, m);
    CHECK(need[i] == (ev ? (uint64_t)permille * (cells_of[i] - 1u) / 1000u + 1u : 0u));
  }
  // in place: floor_db may be the spectrum itself
  std::vector<float> inplace = s;
  CHECK(scn_local_floor_from_spectrum(inplace.data(), n, dc_arg, ub_arg, permille_arg, train, guard, inplace.data()) == SCN_OK);
  for (uint32_t j = 0; j < n; j++) CHECK(bits_of(inplace[j]) == bits_of(bits_of(want[j]) == bits_of(sentinel) ? s[j] : want[j]));
}

int main() {
  const uint32_t permilles[] = {SCN_FLOOR_MIN, 0u, 1u, 750u, 1000u};
  const uint32_t sizes[] = {16u, 17u, 33u, 64u, 257u, 1000u, 1001u};
  const uint32_t windows[][2] = {{1, 0}, {1, 1}, {2, 1}, {16, 2}, {5, 64}, {128, 0}, {128, 64}};
  for (uint32_t n : sizes)
    for (const auto &w : windows)
      for (uint32_t pm : permilles) {
        check_case(n, 0, 0.0, pm, w[0], w[1]);                      // the descriptor's defaults
        check_case(n, SCN_DC_IGNORE_NONE, 1.0, pm, w[0], w[1]);     // every bin evaluated: i_hi = n, past the last index
        check_case(n, 2, 0.5, pm, w[0], w[1]);
      }
  check_case(64, 4, 0.01, 0, 4, 1);  // the mask lets no bin through
  // the limits, and what is refused before anything is read
  std::vector<float> s(64, 1.0f), out(64, 0.0f);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 0, 0, 1, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 0, SCN_FLOOR_TRAIN_MAX + 1u, 0, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 0, 1, SCN_FLOOR_GUARD_MAX + 1u, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 0, 0xffffffffu, 0xffffffffu, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 1001, 4, 1, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(nullptr, 64, 0, 0.0, 0, 4, 1, out.data()) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 64, 0, 0.0, 0, 4, 1, nullptr) == SCN_E_INVALID);
  CHECK(scn_local_floor_from_spectrum(s.data(), 0, 0, 0.0, 0, 4, 1, out.data()) == SCN_E_INVALID);
  // the header's example: n = 16 evaluates i in {2, 3, 4, 12, 13, 14}; (1, 0) is valid, (1, 1) leaves bin 3 without a cell
  std::vector<uint16_t> need;
  uint32_t i_lo = 0, i_hi = 0;
  CHECK(evaluated_bins(16, 4, 0.75, &i_lo, &i_hi) == 6);
  CHECK(floor_window_ranks(16, 4, i_lo, i_hi, 500, 1, 0, need) == SCN_OK);
  CHECK(floor_window_ranks(16, 4, i_lo, i_hi, 500, 1, 1, need) == SCN_E_INVALID && std::strstr(scn_last_error(), "i = 3") != nullptr);
  // no window: the unit-wide floor in every evaluated entry
  float unit_floor = 0.0f;
  const std::vector<float> r = spectrum(1000, 9);
  std::vector<float> fl(1000, -1.0f);
  CHECK(scn_floor_from_spectrum(r.data(), 1000, 0, 0.0, 250, &unit_floor) == SCN_OK);
  CHECK(scn_local_floor_from_spectrum(r.data(), 1000, 0, 0.0, 250, 0, 0, fl.data()) == SCN_OK);
  Mask m = {4, 0, 0};
  evaluated_bins(1000, 4, 0.75, &m.i_lo, &m.i_hi);
  for (uint32_t i = 0; i < 1000; i++) {
    const uint32_t j = (i + 500) % 1000;
    CHECK(bits_of(fl[j]) == bits_of(scn_bin_evaluated(j, i, 1000u, m) ? unit_floor : -1.0f));
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("local floor tests ok\n");
  return 0;
}
