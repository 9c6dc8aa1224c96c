// The arithmetic behind a plan (scanner_amd/csrc/scn_host.hip) as a stand-alone program: built by g++ -x c++ together with that
// unit, no HIP header on the include path, plain and under ASan + UBSan (tests/test_host_cpp.py).  Smallest sizes per branch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
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

static const double kPi = 3.14159265358979323846;
typedef std::vector<double> vec;

// X[k] = sum_j x[j] exp(-2 pi i j k / m), the O(m^2) way
static void naive_dft(const vec &re, const vec &im, vec &out_re, vec &out_im) {
  const size_t m = re.size();
  out_re.assign(m, 0.0);
  out_im.assign(m, 0.0);
  for (size_t k = 0; k < m; k++)
    for (size_t j = 0; j < m; j++) {
      const double a = -2.0 * kPi * (double)((j * k) % m) / (double)m, c = std::cos(a), s = std::sin(a);
      out_re[k] += re[j] * c - im[j] * s;
      out_im[k] += re[j] * s + im[j] * c;
    }
}

// max |a - b| over max |b|
static double rel_to_largest(const vec &a_re, const vec &a_im, const vec &b_re, const vec &b_im) {
  double err = 0.0, top = 0.0;
  for (size_t k = 0; k < b_re.size(); k++) {
    err = std::fmax(err, std::hypot(a_re[k] - b_re[k], a_im[k] - b_im[k]));
    top = std::fmax(top, std::hypot(b_re[k], b_im[k]));
  }
  return err / top;
}

static void test_host_fft() {
  for (size_t m : {2u, 16u, 64u}) {
    vec re(m), im(m), want_re, want_im;
    for (size_t j = 0; j < m; j++) {
      re[j] = std::sin(0.7 * (double)j) + 0.25 * (double)(j % 3);
      im[j] = std::cos(1.3 * (double)j) - 0.5;
    }
    naive_dft(re, im, want_re, want_im);
    host_fft(re, im);
    CHECK(rel_to_largest(re, im, want_re, want_im) <= 1e-12);
  }
}

static void test_twiddles() {
  const std::vector<float> tf = twiddles<float>(16);
  const vec td = twiddles<double>(16);
  CHECK(tf.size() == 32 && td.size() == 32);
  for (uint32_t k = 0; k < 16; k++) {
    const double a = -2.0 * kPi * (double)k / 16.0;
    CHECK(td[2 * k] == std::cos(a) && td[2 * k + 1] == std::sin(a));
    CHECK(tf[2 * k] == (float)std::cos(a) && tf[2 * k + 1] == (float)std::sin(a));  // evaluated in double, rounded once
  }
}

// cosl / sinl of the chirp's exactly reduced angle -pi (i^2 mod 2n) / n: the reduction in uint64_t (i * i passes 2^31 from n = 46342 on)
static const long double kPiL = 3.14159265358979323846264338327950288L;
static void chirp_exact(uint32_t i, uint32_t n, long double &c, long double &s) {
  const uint64_t r = ((uint64_t)i * (uint64_t)i) % (2ull * (uint64_t)n);
  const long double a = -kPiL * (long double)r / (long double)n;
  c = cosl(a);
  s = sinl(a);
}

static void test_bluestein(uint32_t n, uint32_t m_want) {
  const ScnBluesteinTables t = bluestein_tables(n);
  CHECK(t.m == m_want && (1u << t.log2m) == t.m && t.m >= 2 * n - 1 && t.m / 2 < 2 * n - 1);
  CHECK(t.chirp.size() == 2 * (size_t)n && t.bfilter.size() == 2 * (size_t)t.m && t.twiddle.size() == 2 * (size_t)t.m);
  if (g_failed) return;
  CHECK(t.twiddle == twiddles<double>(t.m));
  vec br(t.m, 0.0), bi(t.m, 0.0), want_re, want_im, got_re(t.m), got_im(t.m);
  for (uint32_t i = 0; i < n; i++) {  // w[i] = exp(-i pi i^2 / n), i^2 reduced mod 2n
    long double c, s;
    chirp_exact(i, n, c, s);
    CHECK(fabsl((long double)t.chirp[2 * i] - c) <= 1e-15L && fabsl((long double)t.chirp[2 * i + 1] - s) <= 1e-15L);
    br[i] = br[(t.m - i) % t.m] = (double)c;  // the cyclic conj(w[|k|])
    bi[i] = bi[(t.m - i) % t.m] = -(double)s;
  }
  naive_dft(br, bi, want_re, want_im);
  for (uint32_t k = 0; k < t.m; k++) {
    want_re[k] /= (double)t.m;
    want_im[k] /= (double)t.m;
    got_re[k] = t.bfilter[2 * k];
    got_im[k] = t.bfilter[2 * k + 1];
  }
  CHECK(rel_to_largest(got_re, got_im, want_re, want_im) <= 1e-12);
}

// The sizes at which i * i passes 2^31 (n >= 46342; 46341 is the last below) and comes within 0.006 % of 2^32 (65535): every chirp
// entry against cosl / sinl of the EXACTLY reduced angle -pi (i^2 mod 2n) / n, the reduction in uint64_t; 64 spread bins of the
// filter transform (0, 1, m/2 and m-1 among them) against the direct sum in long double over a long double W_m table.  The full
// naive_dft stays at 17 and 48.
static void test_bluestein_large(uint32_t n) {
  const ScnBluesteinTables t = bluestein_tables(n);
  const uint32_t m = t.m;
  CHECK((1u << t.log2m) == m && m >= 2 * n - 1 && m / 2 < 2 * n - 1 && m == 131072u);
  CHECK(t.chirp.size() == 2 * (size_t)n && t.bfilter.size() == 2 * (size_t)m && t.twiddle.size() == 2 * (size_t)m);
  if (g_failed) return;
  std::vector<long double> br(m, 0.0L), bi(m, 0.0L), wr(m), wi(m);
  double worst = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    long double c, s;
    chirp_exact(i, n, c, s);
    worst = std::fmax(worst, std::fmax((double)fabsl((long double)t.chirp[2 * i] - c), (double)fabsl((long double)t.chirp[2 * i + 1] - s)));
    br[i] = br[(m - i) % m] = c;  // the cyclic conj(w[|k|])
    bi[i] = bi[(m - i) % m] = -s;
  }
  CHECK(worst <= 1e-15);
  for (uint32_t k = 0; k < m; k++) {
    const long double a = -2.0L * kPiL * (long double)k / (long double)m;
    wr[k] = cosl(a);
    wi[k] = sinl(a);
  }
  std::vector<uint32_t> bins = {0u, 1u, m / 2u, m - 1u};
  for (uint32_t s = 1; s <= 60; s++) bins.push_back((uint32_t)(((uint64_t)s * (m - 1u)) / 61u) | 1u);  // odd, so none of the four above but m - 1
  CHECK(bins.size() == 64);
  long double err = 0.0L, top = 0.0L;
  for (uint32_t k : bins) {
    CHECK(k < m);
    long double sr = 0.0L, si = 0.0L;
    for (uint32_t j = 0; j < m; j++) {
      if (j >= n && j <= m - n) continue;  // the zero padding between the two halves of the filter
      const uint32_t e = (uint32_t)(((uint64_t)j * k) & (m - 1u));
      sr += br[j] * wr[e] - bi[j] * wi[e];
      si += br[j] * wi[e] + bi[j] * wr[e];
    }
    sr /= (long double)m;
    si /= (long double)m;
    err = fmaxl(err, hypotl((long double)t.bfilter[2 * k] - sr, (long double)t.bfilter[2 * k + 1] - si));
    top = fmaxl(top, hypotl(sr, si));
  }
  std::printf("bluestein_tables(%u): chirp within %.2e of the exactly reduced angle's, 64 filter bins within %.2Le of the largest\n", n, worst,
              top > 0.0L ? err / top : 0.0L);
  CHECK(top > 0.0L && err <= 1e-12L * top);
}

struct Mask {
  uint32_t dc_ignore, i_lo, i_hi;
};

static void test_evaluated_bins(uint32_t n, uint32_t dc_ignore, double use_bandwidth, bool none) {
  uint32_t i_lo = 1, i_hi = 1;
  const uint32_t kept = evaluated_bins(n, dc_ignore, use_bandwidth, &i_lo, &i_hi);
  const uint32_t use_window = (uint32_t)(use_bandwidth * n / 2.0);
  CHECK(i_lo == n / 2 - use_window && i_hi == n / 2 + use_window);  // (uint32, wrapping)
  const Mask mask = {dc_ignore, n / 2 - use_window, n / 2 + use_window};
  uint32_t brute = 0;
  for (uint32_t i = 0; i < n; i++) brute += scn_bin_evaluated((i + n / 2) % n, i, n, mask) ? 1u : 0u;
  CHECK(kept == brute);
  CHECK(none ? kept == 0 : kept > 0);
  CHECK(evaluated_bins(n, dc_ignore, use_bandwidth, nullptr, nullptr) == kept);
}

static void test_windows() {
  for (uint32_t n : {16u, 17u})
    for (uint32_t type = SCN_WIN_HANN; type <= SCN_WIN_HAMMING; type++) {
      std::vector<float> w;
      CHECK(build_window(type, n, w) && w.size() == n);
      for (uint32_t i = 0; i < n; i++) {
        CHECK(std::memcmp(&w[i], &w[n - 1 - i], sizeof(float)) == 0);
        if (type == SCN_WIN_RECTANGULAR || type == SCN_WIN_KAISER) CHECK(w[i] == 1.0f);
      }
      if (type == SCN_WIN_BLACKMAN_HARRIS && n == 16) CHECK(w[0] == (float)(0.35875 - 0.48829 + 0.14128 - 0.01168) && w[15] == w[0]);
    }
  std::vector<float> w;
  CHECK(!build_window(0, 16, w) && !build_window(SCN_WIN_HAMMING + 1, 16, w));
}

static void test_convert_scale() {
  // tests/test_fused_k1_cpu.py: float(1.0 / intN_t(1 << (enob - 1))), the narrowing wrap included
  CHECK(convert_scale(SCN_KIND_BYTE_COMPLEX, 8) == (float)(1.0 / (double)(int8_t)(1 << 7)) && convert_scale(SCN_KIND_BYTE_COMPLEX, 8) == -1.0f / 128.0f);
  CHECK(convert_scale(SCN_KIND_SHORT_COMPLEX, 16) == (float)(1.0 / (double)(int16_t)(1 << 15)) && convert_scale(SCN_KIND_SHORT, 16) == -1.0f / 32768.0f);
  CHECK(convert_scale(SCN_KIND_SHORT_COMPLEX, 12) == 1.0f / 2048.0f && convert_scale(SCN_KIND_BYTE_COMPLEX, 7) == 1.0f / 64.0f);
  CHECK(convert_scale(SCN_KIND_FLOAT_COMPLEX, 12) == 1.0f);
  CHECK(bytes_per_sample(SCN_KIND_BYTE_COMPLEX) == 2 && bytes_per_sample(SCN_KIND_SHORT) == 4 && bytes_per_sample(SCN_KIND_SHORT_COMPLEX) == 4);
  CHECK(bytes_per_sample(SCN_KIND_FLOAT_COMPLEX) == 8 && bytes_per_sample(0) == 0);
}

// K = 2, G = 3: dwell = buffers {0,1} {2,3} {4,5}; sweeps = buffers {0,3} {1,4} {2,5}
static void test_group_headers() {
  const uint32_t k = 2, ng = 3, nb = k * ng;
  for (int sweeps = 0; sweeps < 2; sweeps++) {
    double fc_in[6];
    uint64_t seq_in[6];
    for (uint32_t b = 0; b < nb; b++) {
      fc_in[b] = 1e6 * (double)(sweeps ? b % ng : b / k);
      seq_in[b] = 100 + b;
    }
    const uint32_t first[3] = {0, sweeps ? 1u : 2u, sweeps ? 2u : 4u};  // each group's first buffer
    CHECK(check_average(k, sweeps != 0, nb, fc_in) == SCN_OK && check_average(k, sweeps != 0, nb, nullptr) == SCN_OK);
    CHECK(check_average(k, sweeps != 0, nb - 1, fc_in) == SCN_E_INVALID && std::strlen(scn_last_error()) > 0);
    for (int with_seq = 0; with_seq < 2; with_seq++)
      for (int with_fc = 0; with_fc < 2; with_fc++) {
        const double *fc = with_fc ? fc_in : nullptr;
        const uint64_t *seq = with_seq ? seq_in : nullptr;
        std::vector<double> group_fc;
        std::vector<uint64_t> group_seq;
        CHECK(group_headers(k, sweeps != 0, nb, fc, seq, group_fc, group_seq) == ng);
        CHECK(with_fc ? fc == group_fc.data() && group_fc.size() == ng : fc == nullptr && group_fc.empty());
        if (!with_seq && sweeps) {  // group g's first buffer is buffer g: the default of a submit without ids
          CHECK(seq == nullptr && group_seq.empty());
        } else {
          CHECK(seq == group_seq.data() && group_seq.size() == ng);
        }
        for (uint32_t g = 0; g < ng && !g_failed; g++) {
          if (with_fc) CHECK(fc[g] == fc_in[first[g]]);
          if (seq) CHECK(seq[g] == (with_seq ? seq_in[first[g]] : (uint64_t)first[g]));
        }
      }
    fc_in[sweeps ? 4 : 3] += 1.0;  // the second buffer of group 1
    CHECK(check_average(k, sweeps != 0, nb, fc_in) == SCN_E_INVALID && std::strstr(scn_last_error(), "group 1") != nullptr);
  }
}

static void test_hackrf_fixup() {
  const uint64_t tuned = 2410000000ull;
  auto frame = [&](uint8_t *t) {
    t[0] = t[1] = 0x7F;
    for (int b = 0; b < 8; b++) t[2 + b] = (uint8_t)(tuned >> (8 * b));
    t[10] = (uint8_t)(int8_t)-7;
    t[11] = 9;
  };
  double fc = 0.0;
  uint32_t mismatch = 99;
  {  // the smallest transfer: exactly the 12 bytes the fix-up reads
    std::unique_ptr<uint8_t[]> t(new uint8_t[12]);
    frame(t.get());
    CHECK(scn_hackrf_sweep_fixup(t.get(), 12, 7500000u, &fc, &mismatch) == SCN_OK && fc == (double)(tuned + 7500000u) && mismatch == 0);
    for (int j = 0; j < 5; j++) CHECK((int8_t)t[2 * j] == -7 && t[2 * j + 1] == 9);
    CHECK((int8_t)t[10] == -7 && t[11] == 9);
    CHECK(scn_hackrf_sweep_fixup(t.get(), 11, 0, &fc, nullptr) == SCN_E_INVALID && scn_hackrf_sweep_fixup(nullptr, 12, 0, &fc, nullptr) == SCN_E_INVALID);
  }
  const uint32_t len = 2 * 16384;  // two blocks of 8192 samples: the second pass looks at the (already patched) head again
  std::unique_ptr<uint8_t[]> t(new uint8_t[len]), before(new uint8_t[len]);
  for (uint32_t b = 0; b < len; b++) t[b] = (uint8_t)(b * 7u + 3u);
  frame(t.get());
  std::memcpy(before.get(), t.get(), len);
  CHECK(scn_hackrf_sweep_fixup(t.get(), len, 0, &fc, &mismatch) == SCN_OK && fc == (double)tuned && mismatch == 0);
  for (int j = 0; j < 5; j++) CHECK((int8_t)t[2 * j] == -7 && t[2 * j + 1] == 9);
  CHECK(std::memcmp(t.get() + 10, before.get() + 10, len - 10) == 0);
  // a fill of (0x7F, 0x7F) leaves the marker standing, so the second block's pass runs too: it reads the patched head as another
  // tuning (one mismatch) and averages the fill with the sample before the block, in int, truncating, narrowed back to int8
  frame(t.get());
  t[10] = t[11] = 0x7F;
  t[2 * 8191] = (uint8_t)(int8_t)-128;  // (127 - 128) / 2 = 0, not -1
  t[2 * 8191 + 1] = 50;                 // (127 + 50) / 2 = 88
  CHECK(scn_hackrf_sweep_fixup(t.get(), len, 5u, &fc, &mismatch) == SCN_OK && mismatch == 1 && fc == (double)(0x7F7F7F7F7F7F7F7Full + 5u));
  for (int j = 0; j < 5; j++) CHECK(t[2 * j] == 0 && t[2 * j + 1] == 88);
  for (uint32_t b = 0; b < len; b++) t[b] = (uint8_t)(b * 7u + 3u);  // (no 0x7F 0x7F at the head)
  std::memcpy(before.get(), t.get(), len);
  CHECK(scn_hackrf_sweep_fixup(t.get(), len, 1234u, &fc, &mismatch) == SCN_OK && fc == 1234.0 && mismatch == 0);
  CHECK(std::memcmp(t.get(), before.get(), len) == 0);
}

static void test_signals_from_hits() {
  // one unit with runs {3,4} {9}, a second unit with {2}: three signals at max_gap 0
  const scn_hit hits[] = {{5, 3, -10.0f, 1003}, {5, 4, -8.0f, 1004}, {5, 9, -20.0f, 1009}, {6, 2, -1.0f, 2002}};
  uint64_t total = 0;
  CHECK(scn_signals_from_hits(hits, 4, 16, 1600, 0, nullptr, 0, &total) == SCN_E_TRUNCATED && total == 3 && std::strlen(scn_last_error()) > 0);
  std::unique_ptr<scn_signal[]> out(new scn_signal[total - 1]);  // (exactly cap records: a write past them is the sanitizer's)
  uint64_t again = 0;
  CHECK(scn_signals_from_hits(hits, 4, 16, 1600, 0, out.get(), total - 1, &again) == SCN_E_TRUNCATED && again == total);
  CHECK(out[0].seq_id == 5 && out[0].first_i == 3 && out[0].last_i == 4 && out[0].peak_i == 4 && out[0].n_hits == 2 && out[0].peak_freq_hz == 1004 &&
        out[0].bandwidth_hz == 200);
  CHECK(out[1].seq_id == 5 && out[1].first_i == 9 && out[1].last_i == 9 && out[1].n_hits == 1 && out[1].peak_power_db == -20.0f);
  std::unique_ptr<scn_signal[]> all(new scn_signal[total]);
  CHECK(scn_signals_from_hits(hits, 4, 16, 1600, 0, all.get(), total, &again) == SCN_OK && again == total && all[2].seq_id == 6 && all[2].first_i == 2);
  CHECK(scn_signals_from_hits(hits, 4, 16, 1600, 4, all.get(), total, &again) == SCN_OK && again == 2 && all[0].last_i == 9 && all[0].n_hits == 3);
}

static void test_floor_from_spectrum() {
  const uint32_t n = 16;
  float power[n];
  for (uint32_t j = 0; j < n; j++) power[j] = -50.0f + 3.5f * (float)((j * 5u) % n) - (j == 3 ? 40.0f : 0.0f);
  uint32_t i_lo = 0, i_hi = 0;
  evaluated_bins(n, 0, 0.75, &i_lo, &i_hi);
  const Mask mask = {0, i_lo, i_hi};
  std::vector<float> kept;
  for (uint32_t i = 0; i < n; i++)
    if (scn_bin_evaluated((i + n / 2) % n, i, n, mask)) kept.push_back(power[(i + n / 2) % n]);
  for (size_t a = 0; a < kept.size(); a++)  // ascending
    for (size_t b = a + 1; b < kept.size(); b++)
      if (kept[b] < kept[a]) std::swap(kept[a], kept[b]);
  CHECK(kept.size() == 13);
  float got = 0.0f;
  CHECK(scn_floor_from_spectrum(power, n, SCN_DC_IGNORE_NONE, 0.75, 0, &got) == SCN_OK && got == kept[500 * (kept.size() - 1) / 1000]);  // the median
  CHECK(scn_floor_from_spectrum(power, n, SCN_DC_IGNORE_NONE, 0.75, 1000, &got) == SCN_OK && got == kept.back());
  CHECK(scn_floor_from_spectrum(power, n, SCN_DC_IGNORE_NONE, 0.75, SCN_FLOOR_MIN, &got) == SCN_OK && got == kept.front());
  CHECK(scn_floor_from_spectrum(power, n, SCN_DC_IGNORE_NONE, 0.75, 1001, &got) == SCN_E_INVALID);
  uint32_t permille = 7;
  CHECK(floor_permille_of(0, &permille) && permille == 500 && floor_permille_of(SCN_FLOOR_MIN, &permille) && permille == 0);
  CHECK(floor_permille_of(1000, &permille) && permille == 1000 && !floor_permille_of(1001, &permille));
}

// The detect kernels' grid (scn_mask.h): ceil(n_units / teams) workgroups, capped at num_cus * per_cu, 256 CUs where the count is unknown
static void test_team_grid() {
  for (int num_cus : {0, 64, 256, 304})
    for (int per_cu : {1, 2, 8}) {
      for (uint32_t nu = 1; nu <= 4; nu++) CHECK(scn_team_grid(nu, 4, num_cus, per_cu) == 1);
      CHECK(scn_team_grid(5, 4, num_cus, per_cu) == 2);
      CHECK(scn_team_grid(9, 1, num_cus, per_cu) == 9);
    }
  CHECK(scn_team_grid(1000000, 4, 256, 8) == 2048);  // capped
  for (int num_cus : {0, -1, -256}) CHECK(scn_team_grid(10000, 1, num_cus, 2) == 512);
  // the largest submit the C-ABI carries: scn_plan_desc.max_batch is a uint32_t with a lower bound only, and a submit may fill it.
  // n_units + teams - 1 would wrap there (to 2, a grid of 0 workgroups): the quotient and the remainder do not.
  const uint32_t max_batch = UINT32_MAX;
  for (int num_cus : {0, 64, 256}) CHECK(scn_team_grid(max_batch, 4, num_cus, 8) == (uint32_t)(num_cus > 0 ? num_cus : 256) * 8u);
  CHECK(scn_team_grid(max_batch, 4, 1 << 20, 1 << 10) == (1u << 30));  // ceil((2^32 - 1) / 4), under a cap that equals it
  for (uint32_t back = 0; back < 3; back++) CHECK(scn_team_grid(max_batch - back, 4, 1 << 20, 1 << 11) == (1u << 30));  // the three that would wrap
  CHECK(scn_team_grid(max_batch - 3u, 4, 1 << 20, 1 << 11) == (1u << 30) - 1u);  // 2^32 - 4: whole workgroups, the last that does not
  CHECK(scn_team_grid(max_batch, 1, 1 << 20, 1 << 11) == (1u << 31));  // capped by 2^31 resident
}

int main() {
  test_host_fft();
  test_twiddles();
  test_bluestein(17, 64);
  test_bluestein(48, 128);
  for (uint32_t n : {46341u, 46342u, 65534u, 65535u}) test_bluestein_large(n);
  test_evaluated_bins(16, 0, 0.75, false);
  test_evaluated_bins(64, 4, 0.75, false);
  test_evaluated_bins(64, 4, 0.01, true);
  test_evaluated_bins(4096, 8, 0.001, true);
  test_windows();
  test_convert_scale();
  test_group_headers();
  test_hackrf_fixup();
  test_signals_from_hits();
  test_floor_from_spectrum();
  test_team_grid();
  CHECK(std::strcmp(scn_error_name(SCN_E_TRUNCATED), "SCN_E_TRUNCATED") == 0 && scn_abi_version() == SCN_ABI_VERSION);
  if (g_failed) return 1;
  std::printf("plan math tests ok\n");
  return 0;
}
