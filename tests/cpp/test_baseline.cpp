// The baseline detector's host arithmetic (scanner_amd/csrc/scn_host.hip: check_baseline_submit, check_baseline_update,
// check_baseline_range; scn_mask.h: scn_baseline_row) as a stand-alone program: built by g++ -x c++ together with that unit, no HIP
// header on the include path, plain and under ASan + UBSan (tests/test_baseline_cpp.py).  The row of a unit against the definition
// written out in 64 bits, at the sizes where the short cut and the division meet and at the top of the 32-bit range; every refusal
// with its status and the statement that follows it.
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

int main() {
  // the row of a unit: (first + u) % rows for every first < rows, over runs that wrap not at all, once and many times
  const uint32_t row_counts[] = {1u, 2u, 3u, 7u, 64u, 1000u};
  for (uint32_t rows : row_counts)
    for (uint32_t first = 0; first < rows; first += (rows > 64u ? 37u : 1u))
      for (uint32_t u = 0; u < 3u * rows + 5u; u++) CHECK(scn_baseline_row(first, u, rows) == (uint32_t)(((uint64_t)first + u) % rows));
  // the top of the range the launchers admit: first + u < 2^32
  CHECK(scn_baseline_row(0xfffffff0u, 0xfu, 0xfffffff1u) == 0xeu);
  CHECK(scn_baseline_row(0x7fffffffu, 0x80000000u, 0x80000000u) == 0x7fffffffu);
  CHECK(scn_baseline_row(0u, 0xffffffffu, 0xffffffffu) == 0u);
  CHECK(scn_baseline_row(0u, 0xfffffffeu, 0xffffffffu) == 0xfffffffeu);
  // a wrapping run of units <= rows names every row at most once: what lets an update write without a race
  for (uint32_t rows : row_counts)
    for (uint32_t first = 0; first < rows; first += (rows > 64u ? 131u : 1u)) {
      std::vector<uint8_t> seen(rows, 0);
      for (uint32_t u = 0; u < rows; u++) {
        const uint32_t r = scn_baseline_row(first, u, rows);
        CHECK(r < rows && !seen[r]);
        if (r < rows) seen[r] = 1;
      }
    }

  // a submit: a plan without rows refuses everything; an indexed one wants a row per table entry, or one row
  CHECK(check_baseline_submit(0, false, 0) == SCN_E_STATE && std::strstr(scn_last_error(), "no baseline") != nullptr);
  CHECK(check_baseline_submit(0, true, 9) == SCN_E_STATE);
  CHECK(check_baseline_submit(1, false, 0) == SCN_OK);
  CHECK(check_baseline_submit(5, false, 9) == SCN_OK);  // (a plain submit reads rows 0 ..., whatever the table holds)
  CHECK(check_baseline_submit(9, true, 9) == SCN_OK);
  CHECK(check_baseline_submit(1, true, 9) == SCN_OK);
  CHECK(check_baseline_submit(1, true, 0) == SCN_OK);
  CHECK(check_baseline_submit(8, true, 9) == SCN_E_STATE && std::strstr(scn_last_error(), "it has 8") != nullptr);
  CHECK(check_baseline_submit(10, true, 9) == SCN_E_STATE);
  CHECK(check_baseline_submit(0xffffffffu, true, 0xfffffffeu) == SCN_E_STATE);

  // an update: a known op, and no more units than rows
  CHECK(check_baseline_update(4, 4, SCN_BASELINE_SET) == SCN_OK);
  CHECK(check_baseline_update(4, 0, SCN_BASELINE_MAX) == SCN_OK);
  CHECK(check_baseline_update(0xffffffffu, 0xffffffffu, SCN_BASELINE_MAX) == SCN_OK);
  CHECK(check_baseline_update(4, 5, SCN_BASELINE_MAX) == SCN_E_INVALID && std::strstr(scn_last_error(), "written twice") != nullptr);
  CHECK(check_baseline_update(1, 7, SCN_BASELINE_SET) == SCN_E_INVALID);
  CHECK(check_baseline_update(4, 4, 2) == SCN_E_INVALID && std::strstr(scn_last_error(), "op 2") != nullptr);
  CHECK(check_baseline_update(4, 4, 0xffffffffu) == SCN_E_INVALID);

  // a read-out: [first_row, first_row + rows) inside the baseline, the sum taken in 64 bits
  CHECK(check_baseline_range(5, 0, 5) == SCN_OK);
  CHECK(check_baseline_range(5, 5, 0) == SCN_OK);
  CHECK(check_baseline_range(5, 4, 1) == SCN_OK);
  CHECK(check_baseline_range(0, 0, 0) == SCN_OK);
  CHECK(check_baseline_range(5, 4, 2) == SCN_E_INVALID && std::strstr(scn_last_error(), "outside") != nullptr);
  CHECK(check_baseline_range(5, 6, 0) == SCN_E_INVALID);
  CHECK(check_baseline_range(0, 0, 1) == SCN_E_INVALID);
  CHECK(check_baseline_range(5, 0xffffffffu, 2) == SCN_E_INVALID);  // (would wrap to 1 in 32 bits)
  CHECK(check_baseline_range(0xffffffffu, 0xfffffffeu, 1) == SCN_OK);
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("baseline tests ok\n");
  return 0;
}
