// The hit history's host arithmetic (scanner_amd/csrc/scn_host.hip: check_history_fold, check_history_window, check_history_range,
// scn_history_fold_hits, scn_confirm_hits; scn_mask.h: scn_history_fold, scn_history_mask, scn_history_confirms) as a stand-alone
// program: built by g++ -x c++ together with that unit, no HIP header on the include path, plain and under ASan + UBSan
// (tests/test_history_cpp.py).  The mask at every window -- 32 is the one a shift cannot make --, the predicate against a popcount
// written out bit by bit, every refusal with its status, and both host forms on lists small enough to read: rows that wrap, an
// empty unit, a row that no unit maps to, visits that stop at 0xffffffff, bits that fall off the top of the word.
#include <cstdio>
#include <cstring>
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

static scn_hit hit(uint64_t seq, uint32_t i) {
  scn_hit h;
  std::memset(&h, 0, sizeof(h));
  h.seq_id = seq;
  h.i = i;
  h.power_db = 1.0f + (float)i;
  h.freq_hz = 100u + i;
  return h;
}

static uint32_t bits_set(uint32_t w) {
  uint32_t c = 0;
  for (int k = 0; k < 32; k++) c += (w >> k) & 1u;
  return c;
}

int main() {
  // the mask: the `window` lowest bits, all 32 at 32 (1u << 32 is not a shift C++ defines)
  for (uint32_t window = 1; window <= 32; window++) {
    const uint32_t mask = scn_history_mask(window);
    CHECK(bits_set(mask) == window && (mask & 1u) == 1u && (window == 32 || (mask >> window) == 0u));
  }
  CHECK(scn_history_mask(32) == 0xffffffffu && scn_history_mask(31) == 0x7fffffffu && scn_history_mask(1) == 1u);
  // the fold: the visit comes in at bit 0, only bit 0 of `hit` counts, bit 31 falls off
  CHECK(scn_history_fold(0u, 1u) == 1u && scn_history_fold(1u, 0u) == 2u && scn_history_fold(0x80000001u, 1u) == 3u);
  CHECK(scn_history_fold(0xffffffffu, 0u) == 0xfffffffeu && scn_history_fold(5u, 0xfffffffeu) == 10u && scn_history_fold(5u, 0xffffffffu) == 11u);
  // the predicate: popcount(word & mask) >= m
  const uint32_t words[] = {0u, 1u, 2u, 0x80000000u, 0xffffffffu, 0x7fffffffu, 0xfffffffeu, 0xaaaaaaaau, 0x00010001u, 0b10110u};
  for (uint32_t word : words)
    for (uint32_t window = 1; window <= 32; window++)
      for (uint32_t m = 1; m <= window; m++)
        CHECK(scn_history_confirms(word, scn_history_mask(window), m) == (bits_set(word & scn_history_mask(window)) >= m));
  CHECK(scn_history_confirms(0xffffffffu, scn_history_mask(32), 32) && !scn_history_confirms(0x7fffffffu, scn_history_mask(32), 32));
  CHECK(scn_history_confirms(0x80000000u, scn_history_mask(32), 1) && !scn_history_confirms(0x80000000u, scn_history_mask(31), 1));

  // (m, window): 1 <= m <= window <= 32
  CHECK(check_history_window(1, 1) == SCN_OK && check_history_window(32, 32) == SCN_OK && check_history_window(1, 32) == SCN_OK);
  CHECK(check_history_window(0, 1) == SCN_E_INVALID && std::strstr(scn_last_error(), "m 0") != nullptr);
  CHECK(check_history_window(0, 0) == SCN_E_INVALID && check_history_window(3, 2) == SCN_E_INVALID);
  CHECK(check_history_window(1, 33) == SCN_E_INVALID && check_history_window(33, 33) == SCN_E_INVALID);
  CHECK(check_history_window(0xffffffffu, 0xffffffffu) == SCN_E_INVALID);
  // a fold: a history, no more units than rows, and for an indexed submit a row per table entry or one row -- in this order
  CHECK(check_history_fold(0, 0, false, 0) == SCN_E_STATE && std::strstr(scn_last_error(), "no hit history") != nullptr);
  CHECK(check_history_fold(0, 9, true, 3) == SCN_E_STATE);
  CHECK(check_history_fold(4, 4, false, 0) == SCN_OK && check_history_fold(4, 0, false, 9) == SCN_OK);
  CHECK(check_history_fold(4, 5, false, 0) == SCN_E_INVALID && std::strstr(scn_last_error(), "visited twice") != nullptr);
  CHECK(check_history_fold(4, 5, true, 9) == SCN_E_INVALID);  // (the same status check_baseline_update gives for that fault)
  CHECK(check_baseline_update(4, 5, SCN_BASELINE_SET) == SCN_E_INVALID);
  CHECK(check_history_fold(9, 3, true, 9) == SCN_OK && check_history_fold(1, 1, true, 9) == SCN_OK);
  CHECK(check_history_fold(8, 3, true, 9) == SCN_E_STATE && std::strstr(scn_last_error(), "it has 8") != nullptr);
  CHECK(check_history_fold(8, 3, false, 9) == SCN_OK);  // (a plain submit visits rows 0 ..., whatever the table holds)
  // a read-out: [first_row, first_row + rows) inside the history, the sum taken in 64 bits
  CHECK(check_history_range(5, 0, 5) == SCN_OK && check_history_range(5, 5, 0) == SCN_OK && check_history_range(0, 0, 0) == SCN_OK);
  CHECK(check_history_range(5, 4, 2) == SCN_E_INVALID && std::strstr(scn_last_error(), "outside") != nullptr);
  CHECK(check_history_range(5, 0xffffffffu, 2) == SCN_E_INVALID && check_history_range(0, 0, 1) == SCN_E_INVALID);

  // the fold on a list: rows 3, n 8, first 2 -> units 0, 1, 2 have rows 2, 0, 1; unit 1 is empty
  const uint32_t rows = 3, n = 8;
  std::vector<uint32_t> history(rows * n, 0u), visits(rows, 0u);
  visits[2] = 0xfffffffeu;  // one visit below the top
  history[2 * n + 7] = 0xc0000001u;
  const uint64_t ids[] = {40, 41, 42};
  const scn_hit list[] = {hit(40, 0), hit(40, 7), hit(42, 3)};
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 2, 3, ids, list, 3) == SCN_OK);
  CHECK(history[2 * n + 0] == 1u && history[2 * n + 7] == 0x80000003u && history[2 * n + 3] == 0u && history[1 * n + 3] == 1u);
  CHECK(visits[0] == 1u && visits[1] == 1u && visits[2] == 0xffffffffu);
  for (uint32_t i = 0; i < n; i++) CHECK(history[0 * n + i] == 0u);  // the empty unit's row: a visit of zeros
  // again, two units only (rows 2 and 0): row 1 is untouched, row 2's visits stay at the top, bit 31 falls off
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 2 + 5 * rows, 2, ids, list, 2) == SCN_OK);  // (first is reduced modulo rows)
  CHECK(history[2 * n + 0] == 3u && history[2 * n + 7] == 7u && history[1 * n + 3] == 1u);
  CHECK(visits[0] == 2u && visits[1] == 1u && visits[2] == 0xffffffffu);
  // without ids a unit's id is its index
  std::vector<uint32_t> h1(n, 0u), v1(1, 0u);
  const scn_hit plain[] = {hit(0, 1), hit(0, 2)};
  for (int visit = 0; visit < 34; visit++) CHECK(scn_history_fold_hits(h1.data(), v1.data(), 1, n, 0, 1, nullptr, plain, visit < 33 ? 2 : 0) == SCN_OK);
  CHECK(h1[1] == 0xfffffffeu && h1[2] == 0xfffffffeu && h1[0] == 0u && v1[0] == 34u);

  // the confirmation: the list's subsequence, the same records, in order
  scn_hit out[4];
  uint64_t n_out = 99;
  CHECK(scn_confirm_hits(history.data(), rows, n, 2, 3, ids, list, 3, 2, 2, out, 4, &n_out) == SCN_OK && n_out == 2);  // row 1 has been visited once
  CHECK(std::memcmp(&out[0], &list[0], sizeof(scn_hit)) == 0 && std::memcmp(&out[1], &list[1], sizeof(scn_hit)) == 0);
  CHECK(scn_confirm_hits(history.data(), rows, n, 2, 3, ids, list, 3, 3, 3, out, 4, &n_out) == SCN_OK && n_out == 1 && out[0].i == 7u);
  CHECK(scn_confirm_hits(history.data(), rows, n, 2, 3, ids, list, 3, 1, 2, out, 4, &n_out) == SCN_OK && n_out == 3);
  CHECK(scn_confirm_hits(history.data(), rows, n, 2, 3, ids, list, 3, 1, 2, out, 2, &n_out) == SCN_E_TRUNCATED && n_out == 3 && out[1].i == 7u);
  CHECK(scn_confirm_hits(history.data(), rows, n, 2, 3, ids, list, 3, 1, 2, nullptr, 0, &n_out) == SCN_E_TRUNCATED && n_out == 3);
  CHECK(scn_confirm_hits(h1.data(), 1, n, 0, 1, nullptr, plain, 2, 32, 32, out, 4, &n_out) == SCN_OK && n_out == 0);   // 31 of 32
  CHECK(scn_confirm_hits(h1.data(), 1, n, 0, 1, nullptr, plain, 2, 31, 32, out, 4, &n_out) == SCN_OK && n_out == 2);
  h1[1] = 0xffffffffu;
  CHECK(scn_confirm_hits(h1.data(), 1, n, 0, 1, nullptr, plain, 2, 32, 32, out, 4, &n_out) == SCN_OK && n_out == 1 && out[0].i == 1u);

  // the refusals leave everything as it was
  const std::vector<uint32_t> before = history, visits_before = visits;
  const scn_hit stray[] = {hit(40, 0), hit(99, 1)};
  const scn_hit late[] = {hit(41, 0), hit(40, 1)};
  const scn_hit wide[] = {hit(40, 0), hit(41, n)};
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 0, 2, ids, stray, 2) == SCN_E_INVALID);
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 0, 2, ids, late, 2) == SCN_E_INVALID);
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 0, 2, ids, wide, 2) == SCN_E_INVALID && std::strstr(scn_last_error(), "outside") != nullptr);
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 0, 0, ids, list, 1) == SCN_E_INVALID);
  CHECK(scn_history_fold_hits(history.data(), visits.data(), rows, n, 0, 4, nullptr, list, 0) == SCN_E_INVALID);  // units > rows
  CHECK(scn_history_fold_hits(history.data(), visits.data(), 0, n, 0, 0, nullptr, list, 0) == SCN_E_INVALID);
  CHECK(scn_history_fold_hits(nullptr, visits.data(), rows, n, 0, 0, nullptr, list, 0) == SCN_E_INVALID);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, stray, 2, 1, 1, out, 4, &n_out) == SCN_E_INVALID && n_out == 0);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, wide, 2, 1, 1, out, 4, &n_out) == SCN_E_INVALID);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, list, 2, 0, 1, out, 4, &n_out) == SCN_E_INVALID);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, list, 2, 2, 1, out, 4, &n_out) == SCN_E_INVALID);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, list, 2, 1, 33, out, 4, &n_out) == SCN_E_INVALID);
  CHECK(scn_confirm_hits(history.data(), rows, n, 0, 2, ids, list, 2, 1, 1, nullptr, 4, &n_out) == SCN_E_INVALID);
  CHECK(history == before && visits == visits_before);
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("history tests ok\n");
  return 0;
}
