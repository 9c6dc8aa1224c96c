// scn_host.hip -- the part of the C-ABI layer that never touches HIP: the error text, what a descriptor resolves to, the tables, the
// entry points that are host arithmetic only.  Plain C++17: no HIP header here or in scn_host.h (tests/cpp/test_plan_math.cpp and
// test_plan_resolve.cpp build the unit with g++ under the sanitizers); the .hip suffix only puts it through the library's compiler.
#include "scn_host.h"

#include "scn_emitters.h"
#include "scn_levels.h"
#include "scn_trace.h"
#include "scn_wire.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

static thread_local std::string g_last_error;

int scn_fail(int status, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return status;
}

size_t bytes_per_sample(uint32_t kind) { return scn_wire_bytes(kind); }

// `int16_t max = 1 << (enob - 1); float onebymax = float(1.0/max);` (utility.cpp:64-65,
// :16-17) and the int8_t flavour (utility.cpp:40-41), including the narrowing wrap that
// makes enob == width give a negative scale.
float convert_scale(uint32_t kind, uint32_t enob) {
  uint32_t one = 1u << ((enob - 1u) & 31u);
  if (kind == SCN_KIND_BYTE_COMPLEX) return (float)(1.0 / (double)(int8_t)(uint8_t)one);
  if (kind == SCN_KIND_SHORT || kind == SCN_KIND_SHORT_COMPLEX) return (float)(1.0 / (double)(int16_t)(uint16_t)one);
  return 1.0f;
}

// gr::fft::window::build(type, N, 0.0) as process.cpp:18 calls it ([3P], GNU Radio 3.7 / 3.8): the published definitions --
// cosine sums with the symmetric denominator N - 1 (Hamming 0.54 / 0.46, Hann 0.5 / 0.5, Blackman 0.42 / 0.5 / 0.08, 4-term
// Blackman-Harris 0.35875 / 0.48829 / 0.14128 / 0.01168, flat-top 1 / 1.93 / 1.29 / 0.388 / 0.028 over 4.63867), the triangular
// Bartlett window, Kaiser with the beta the call passes (0.0: I0(0) / I0(0) = 1 everywhere) -- evaluated in double, stored float.
// scan.cpp:215 only ever asks for Blackman-Harris.
bool build_window(uint32_t type, uint32_t n, std::vector<float> &w) {
  w.resize(n);
  const double pi = 3.14159265358979323846, m = (double)n - 1.0, flat = 4.63867;
  double c[5] = {0, 0, 0, 0, 0};
  switch (type) {
    case SCN_WIN_HAMMING: c[0] = 0.54; c[1] = 0.46; break;
    case SCN_WIN_HANN: c[0] = 0.5; c[1] = 0.5; break;
    case SCN_WIN_BLACKMAN: c[0] = 0.42; c[1] = 0.5; c[2] = 0.08; break;
    case SCN_WIN_RECTANGULAR:
    case SCN_WIN_KAISER:
      std::fill(w.begin(), w.end(), 1.0f);
      return true;
    case SCN_WIN_BLACKMAN_HARRIS: c[0] = 0.35875; c[1] = 0.48829; c[2] = 0.14128; c[3] = 0.01168; break;
    case SCN_WIN_BARTLETT:
      for (uint32_t i = 0; i < n; i++) w[i] = (float)(i < n / 2 ? 2.0 * (double)i / m : 2.0 - 2.0 * (double)i / m);
      return true;
    case SCN_WIN_FLATTOP: c[0] = 1.0 / flat; c[1] = 1.93 / flat; c[2] = 1.29 / flat; c[3] = 0.388 / flat; c[4] = 0.028 / flat; break;
    default: return false;
  }
  for (uint32_t i = 0; i < n; i++) {
    const double x = (double)i / m;
    w[i] = (float)(c[0] - c[1] * std::cos(2.0 * pi * x) + c[2] * std::cos(4.0 * pi * x) - c[3] * std::cos(6.0 * pi * x) + c[4] * std::cos(8.0 * pi * x));
  }
  return true;
}

// In-place forward DFT of a power-of-two length in double (plan creation only: the Bluestein filter's transform).
void host_fft(std::vector<double> &re, std::vector<double> &im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; i++) {  // bit reversal
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  const double pi = 3.14159265358979323846;
  for (size_t len = 2; len <= n; len <<= 1) {
    for (size_t k = 0; k < len / 2; k++) {
      const double a = -2.0 * pi * (double)k / (double)len, wr = std::cos(a), wi = std::sin(a);
      for (size_t i = k; i < n; i += len) {
        const size_t j = i + len / 2;
        const double xr = re[j] * wr - im[j] * wi, xi = re[j] * wi + im[j] * wr;
        re[j] = re[i] - xr;
        im[j] = im[i] - xi;
        re[i] += xr;
        im[i] += xi;
      }
    }
  }
}

template <class T>
std::vector<T> twiddles(uint32_t m) {
  std::vector<T> tw(2 * (size_t)m);
  const double pi = 3.14159265358979323846;
  for (uint32_t k = 0; k < m; k++) {
    const double a = -2.0 * pi * (double)k / (double)m;
    tw[2 * k] = (T)std::cos(a);
    tw[2 * k + 1] = (T)std::sin(a);
  }
  return tw;
}
template std::vector<float> twiddles<float>(uint32_t);
template std::vector<double> twiddles<double>(uint32_t);

// The tables of a Bluestein plan.  The transform length m: the power of two >= 2n - 1; w[i] = exp(-i pi i^2 / n) with i^2 reduced
// mod 2n in integers; the filter b[k] = conj(w[|k|]) laid out cyclically over m points, transformed here in double (m <= 131072)
// and scaled by 1/m (the second device transform is an inverse one up to conjugations, which needs that factor)
ScnBluesteinTables bluestein_tables(uint32_t n) {
  ScnBluesteinTables t;
  for (t.log2m = 0; (1u << t.log2m) < 2u * n - 1u; t.log2m++) {
  }
  const uint32_t m = t.m = 1u << t.log2m;
  const double pi = 3.14159265358979323846;
  std::vector<double> br(m, 0.0), bi(m, 0.0);
  t.chirp.resize(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    // exp(+i pi r / n), r = i^2 mod 2n, with the angle folded into [0, pi/2] in integers first: cos(2 pi - x) = cos x, sin(2 pi - x)
    // = -sin x, then cos(pi - x) = -cos x, sin(pi - x) = sin x.  The double product pi r / n of an r near 2n is itself up to 1.2e-15
    // off (five epsilons, measured at n = 46341: tests/cpp/test_plan_math.cpp); folded, every entry is within 6e-16 of the exact one.
    uint64_t r = ((uint64_t)i * i) % (2ull * n);
    const bool lower = r > n;
    if (lower) r = 2ull * n - r;
    const bool left = 2ull * r > n;
    if (left) r = n - r;
    const double a = pi * (double)r / (double)n;
    const double c = left ? -std::cos(a) : std::cos(a), s = lower ? -std::sin(a) : std::sin(a);
    t.chirp[2 * i] = c;  // w[i] = exp(-i pi r / n)
    t.chirp[2 * i + 1] = -s;
    br[i] = c;
    bi[i] = s;
    if (i) {
      br[m - i] = br[i];
      bi[m - i] = bi[i];
    }
  }
  host_fft(br, bi);
  t.bfilter.resize(2 * (size_t)m);
  for (uint32_t k = 0; k < m; k++) {
    t.bfilter[2 * k] = br[k] / (double)m;
    t.bfilter[2 * k + 1] = bi[k] / (double)m;
  }
  t.twiddle = twiddles<double>(m);
  return t;
}

// rows p = 1 ... `rows` of `threads` entries, each W_n^((stride t p) mod n) as twiddles<float>(n) holds it
std::vector<float> fused_tw1_table(uint32_t n, uint32_t rows, uint32_t threads, uint32_t stride) {
  const std::vector<float> tw = twiddles<float>(n);
  std::vector<float> out(2 * (size_t)rows * threads);
  for (uint32_t p = 1; p <= rows; p++)
    for (uint32_t t = 0; t < threads; t++) {
      const uint32_t k = (uint32_t)(((uint64_t)stride * t * p) % n);
      out[2 * ((size_t)(p - 1) * threads + t)] = tw[2 * k];
      out[2 * ((size_t)(p - 1) * threads + t) + 1] = tw[2 * k + 1];
    }
  return out;
}

ScnAvgHalfTables avg_half_tables() {
  ScnAvgHalfTables t;
  t.half = fused_tw1_table(8192, 15, 256, 2);  // W_4096^(t p) = W_8192^(2 t p)
  t.join = twiddles<double>(8192);
  t.join.resize(8192);  // k < 4096
  return t;
}

// scn_plan_desc.floor_permille with its default applied (0 -> 500, SCN_FLOOR_MIN -> 0); false for a value outside the descriptor's
bool floor_permille_of(uint32_t given, uint32_t *permille) {
  if (given == SCN_FLOOR_MIN) *permille = 0;
  else if (given == 0) *permille = 500;
  else if (given <= 1000u) *permille = given;
  else return false;
  return true;
}

// The mask of process.cpp:46-52 exactly as the kernels apply it (uint32 arithmetic), with the descriptor's defaults already
// applied: i_lo / i_hi, and the number of natural bins it lets through
uint32_t evaluated_bins(uint32_t n, uint32_t dc_ignore, double use_bandwidth, uint32_t *i_lo, uint32_t *i_hi) {
  // process.cpp:85 m_useWindow = uint32_t(useBandWidth * numSamples / 2.0); :51 bounds in uint32
  const uint32_t use_window = (uint32_t)(use_bandwidth * n / 2.0);
  const struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore, n / 2 - use_window, n / 2 + use_window};
  uint32_t kept = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = (i + n / 2) % n;
    kept += scn_bin_evaluated(j, i, n, mask);
  }
  if (i_lo) *i_lo = mask.i_lo;
  if (i_hi) *i_hi = mask.i_hi;
  return kept;
}

int resolve_plan(const scn_plan_desc *desc, PlanShape *out) {
  if (desc->struct_size != sizeof(scn_plan_desc))
    return scn_fail(SCN_E_INVALID, "scn_plan_desc.struct_size %u != %zu (ABI mismatch)", desc->struct_size, sizeof(scn_plan_desc));
  PlanShape s;
  scn_plan_desc &d = s.d = *desc;
  if (!d.window_type) d.window_type = SCN_WIN_BLACKMAN_HARRIS;
  if (!d.mode) d.mode = SCN_MODE_FREQUENCY_DOMAIN;
  if (!d.dc_ignore_bins) d.dc_ignore_bins = 4;  // process.cpp:87
  if (d.dc_ignore_bins == SCN_DC_IGNORE_NONE) d.dc_ignore_bins = 0;
  if (d.use_bandwidth == 0.0) d.use_bandwidth = 0.75;  // scan.cpp:65
  if (!d.trigger_count) d.trigger_count = 1047;        // process.cpp:62
  if (!(d.flags & (SCN_OUT_SPECTRUM | SCN_OUT_HITS))) d.flags |= SCN_OUT_SPECTRUM | SCN_OUT_HITS;
  if (!d.max_batch) return scn_fail(SCN_E_INVALID, "max_batch must be >= 1");
  if (!d.max_hits) d.max_hits = (uint32_t)std::min<uint64_t>((uint64_t)d.max_batch * 64u, 1u << 28);
  if (bytes_per_sample(d.sample_kind) == 0) return scn_fail(SCN_E_INVALID, "unknown sample_kind %u", d.sample_kind);
  if (d.sample_kind != SCN_KIND_FLOAT_COMPLEX && (d.enob < 1 || d.enob > 32)) return scn_fail(SCN_E_INVALID, "enob %u out of range", d.enob);
  if (d.window_type < SCN_WIN_HANN || d.window_type > SCN_WIN_HAMMING) return scn_fail(SCN_E_INVALID, "unsupported window_type %u", d.window_type);
  if (d.mode != SCN_MODE_FREQUENCY_DOMAIN && d.mode != SCN_MODE_TIME_DOMAIN) return scn_fail(SCN_E_INVALID, "unsupported mode %u", d.mode);
  s.path = path_of(d.mode, d.n);
  if (s.path == Path::Unsupported) return scn_fail(SCN_E_INVALID, "unsupported FFT size %u (16 to 65536)", d.n);
  if (d.n == 0 || d.n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad sample count %u", d.n);
  if (d.sample_rate == 0) return scn_fail(SCN_E_INVALID, "sample_rate must be > 0");
  s.avg = d.average ? d.average : 1u;
  if (s.avg > 1u) {
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "average %u needs a frequency-domain plan", s.avg);
    if (!scn_avg_size_supported(d.n)) return scn_fail(SCN_E_INVALID, "average %u: n = %u is not supported (1024, 2048, 4096, 8192)", s.avg, d.n);
    if (d.max_batch % s.avg) return scn_fail(SCN_E_INVALID, "average %u does not divide max_batch %u", s.avg, d.max_batch);
    if (d.average_layout != SCN_AVG_DWELL && d.average_layout != SCN_AVG_SWEEPS) return scn_fail(SCN_E_INVALID, "unknown average_layout %u", d.average_layout);
  }
  const uint32_t kept = evaluated_bins(d.n, d.dc_ignore_bins, d.use_bandwidth, &s.i_lo, &s.i_hi);
  if (d.detect != SCN_DETECT_FIXED && d.detect != SCN_DETECT_FLOOR && d.detect != SCN_DETECT_BASELINE) return scn_fail(SCN_E_INVALID, "unknown detect %u", d.detect);
  if (d.detect == SCN_DETECT_BASELINE) {  // (floor_permille is not read)
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_BASELINE needs a frequency-domain plan");
    // (the caller's own flags: a baseline plan names its outputs, the default of "neither -> both" does not apply to it)
    if (!(desc->flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_BASELINE needs SCN_OUT_HITS set in flags");
  }
  if (d.detect == SCN_DETECT_FLOOR) {
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR needs a frequency-domain plan");
    if (!(d.flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR needs SCN_OUT_HITS");
    if (!floor_permille_of(d.floor_permille, &s.floor_permille))
      return scn_fail(SCN_E_INVALID, "floor_permille %u: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN", d.floor_permille);
    if (!kept) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR: the mask (dc_ignore_bins, use_bandwidth) lets no bin through");
  }
  s.avg_layout = s.avg > 1u ? d.average_layout : (uint32_t)SCN_AVG_DWELL;
  s.buf_bytes = bytes_per_sample(d.sample_kind) * d.n;
  s.scale = convert_scale(d.sample_kind, d.enob);
  s.hit_region = std::max<uint32_t>(kept, 1u);
  s.floor = d.detect == SCN_DETECT_FLOOR;
  if (s.floor) s.floor_rank = (uint32_t)((uint64_t)s.floor_permille * (kept - 1u) / 1000u);
  s.baseline = d.detect == SCN_DETECT_BASELINE;
  s.direct_counts = d.n >= 8192 && (s.path == Path::FusedPow2 || s.path == Path::FusedMixed);
  *out = s;
  return SCN_OK;
}

int resolve_welch(const scn_welch_desc *desc, WelchShape *out) {
  if (desc->struct_size != sizeof(scn_welch_desc)) return scn_fail(SCN_E_INVALID, "scn_welch_desc.struct_size mismatch");
  WelchShape s;
  scn_welch_desc &d = s.d = *desc;
  if (!d.window_type) d.window_type = SCN_WIN_BLACKMAN_HARRIS;
  // (sample_kind, enob, correct_dc were reserved words until ABI version 5: a version-4 caller's zeros mean float samples)
  if (!d.sample_kind) d.sample_kind = SCN_KIND_FLOAT_COMPLEX;
  if (d.sample_kind < SCN_KIND_BYTE_COMPLEX || d.sample_kind > SCN_KIND_FLOAT_COMPLEX) return scn_fail(SCN_E_INVALID, "unsupported sample_kind %u", d.sample_kind);
  if (!d.enob) d.enob = d.sample_kind == SCN_KIND_BYTE_COMPLEX ? 8u : 12u;
  if (d.sample_kind != SCN_KIND_FLOAT_COMPLEX && (d.enob < 1 || d.enob > (d.sample_kind == SCN_KIND_BYTE_COMPLEX ? 8u : 16u)))
    return scn_fail(SCN_E_INVALID, "enob %u out of range for sample_kind %u", d.enob, d.sample_kind);
  if (d.n != 65536) return scn_fail(SCN_E_INVALID, "unsupported Welch segment length %u (65536)", d.n);
  if (d.segments_per_psd < 1 || d.max_psd < 1) return scn_fail(SCN_E_INVALID, "segments_per_psd and max_psd must be >= 1");
  if (d.window_type < SCN_WIN_HANN || d.window_type > SCN_WIN_HAMMING) return scn_fail(SCN_E_INVALID, "unsupported window_type %u", d.window_type);
  s.hop = d.n / 2;
  s.bytes_per_sample = (uint32_t)bytes_per_sample(d.sample_kind);
  s.scale = convert_scale(d.sample_kind, d.enob);
  s.dc = d.correct_dc && d.sample_kind != SCN_KIND_FLOAT_COMPLEX;
  *out = s;
  return SCN_OK;
}

// enough row workgroups for one per CU: 16 tiles x max_psd x parts >= CUs, parts <= 4 and <= K (measured, 8 PSDs per
// submit: 68.5 / 75.9 / 73.7 Gsamples/s with 1 / 2 / 4 parts; from 16 PSDs per submit up the split only costs)
uint32_t welch_parts(uint32_t max_psd, uint32_t segments_per_psd, int num_cus) {
  uint32_t parts = 1;
  while (parts < 4u && parts * 2u <= segments_per_psd && 16u * max_psd * parts < (uint32_t)num_cus) parts *= 2u;
  return parts;
}

int floor_window_ranks(uint32_t n, uint32_t dc_ignore, uint32_t i_lo, uint32_t i_hi, uint32_t permille, uint32_t train, uint32_t guard,
                       std::vector<uint16_t> &need) {
  if (train == 0 || train > SCN_FLOOR_TRAIN_MAX)
    return scn_fail(SCN_E_INVALID, "floor window: train_bins %u outside 1 ... %u", train, SCN_FLOOR_TRAIN_MAX);
  if (guard > SCN_FLOOR_GUARD_MAX) return scn_fail(SCN_E_INVALID, "floor window: guard_bins %u > %u", guard, SCN_FLOOR_GUARD_MAX);
  const struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore, i_lo, i_hi};
  std::vector<uint32_t> before((size_t)n + 1u);  // before[i] = evaluated bins among the fftshift indices [0, i)
  before[0] = 0;
  for (uint32_t i = 0; i < n; i++) before[i + 1] = before[i] + (scn_bin_evaluated((i + n / 2) % n, i, n, mask) ? 1u : 0u);
  // evaluated bins in [lo, hi] clipped to [0, n): no wrap between the band edges
  auto cells = [&](int64_t lo, int64_t hi) -> uint32_t {
    lo = std::max<int64_t>(lo, 0);
    hi = std::min<int64_t>(hi, (int64_t)n - 1);
    return lo > hi ? 0u : before[(size_t)hi + 1u] - before[(size_t)lo];
  };
  need.assign(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (before[i + 1] == before[i]) continue;
    const int64_t c = i, reach = (int64_t)guard + train;
    const uint32_t m = cells(c - reach, c - guard - 1) + cells(c + guard + 1, c + reach);
    if (!m)
      return scn_fail(SCN_E_INVALID, "floor window (train %u, guard %u): the evaluated bin i = %u of %u has no reference cell", train, guard, i, n);
    need[i] = (uint16_t)((uint64_t)permille * (m - 1u) / 1000u + 1u);  // (m <= 2 SCN_FLOOR_TRAIN_MAX)
  }
  return SCN_OK;
}

int check_baseline_submit(uint32_t rows, bool indexed, uint32_t table_count) {
  if (!rows) return scn_fail(SCN_E_STATE, "the plan has no baseline: scn_plan_set_baseline was never called, or dropped it");
  if (indexed && rows != 1u && rows != table_count)
    return scn_fail(SCN_E_STATE, "an indexed submit needs a baseline of 1 row or of one per table entry (%u): it has %u", table_count, rows);
  return SCN_OK;
}

int check_baseline_update(uint32_t rows, uint32_t units, uint32_t op) {
  if (op != SCN_BASELINE_SET && op != SCN_BASELINE_MAX) return scn_fail(SCN_E_INVALID, "unknown baseline op %u", op);
  if (units > rows) return scn_fail(SCN_E_INVALID, "the submit had %u units, the baseline has %u rows: a row would be written twice", units, rows);
  return SCN_OK;
}

int check_baseline_range(uint32_t have, uint32_t first_row, uint32_t rows) {
  if ((uint64_t)first_row + rows > have) return scn_fail(SCN_E_INVALID, "rows [%u, %u + %u) outside the baseline of %u rows", first_row, first_row, rows, have);
  return SCN_OK;
}

int check_history_fold(uint32_t rows, uint32_t units, bool indexed, uint32_t table_count) {
  if (!rows) return scn_fail(SCN_E_STATE, "the plan has no hit history: scn_plan_set_history was never called, or dropped it");
  if (units > rows) return scn_fail(SCN_E_INVALID, "the submit had %u units, the history has %u rows: a row would be visited twice", units, rows);
  if (indexed && rows != 1u && rows != table_count)
    return scn_fail(SCN_E_STATE, "an indexed submit needs a history of 1 row or of one per table entry (%u): it has %u", table_count, rows);
  return SCN_OK;
}

int check_history_window(uint32_t m, uint32_t window) {
  if (m < 1u || m > window || window > 32u) return scn_fail(SCN_E_INVALID, "confirmation needs 1 <= m <= window <= 32: m %u, window %u", m, window);
  return SCN_OK;
}

int check_history_range(uint32_t have, uint32_t first_row, uint32_t rows) {
  if ((uint64_t)first_row + rows > have) return scn_fail(SCN_E_INVALID, "rows [%u, %u + %u) outside the history of %u rows", first_row, first_row, rows, have);
  return SCN_OK;
}

int check_trace_geometry(uint32_t cell_hz, uint32_t cells) {
  if (cell_hz == 0) return scn_fail(SCN_E_INVALID, "a trace cell is at least 1 Hz wide");
  if (cells == 0 || cells > SCN_TRACE_CELLS_MAX) return scn_fail(SCN_E_INVALID, "a trace has 1 ... %u cells: %u", SCN_TRACE_CELLS_MAX, cells);
  return SCN_OK;
}

int check_trace_range(uint32_t have, uint32_t first_cell, uint32_t cells) {
  if ((uint64_t)first_cell + cells > have) return scn_fail(SCN_E_INVALID, "cells [%u, %u + %u) outside the trace of %u cells", first_cell, first_cell, cells, have);
  return SCN_OK;
}

int check_emitters_line(uint32_t line, float threshold_db) {
  if (line > kEmitLineSpread) return scn_fail(SCN_E_INVALID, "line %u: SCN_TRACE_LINE_MAX, _MIN or _SPREAD", line);
  if (scn_trace_is_nan(scn_emit_bits(threshold_db))) return scn_fail(SCN_E_INVALID, "threshold_db is a NaN");
  return SCN_OK;
}

int check_levels_geometry(uint32_t cell_hz, uint32_t cells, uint32_t n_edges) {
  if (int st = check_trace_geometry(cell_hz, cells)) return st;
  if (n_edges == 0 || n_edges > SCN_LEVELS_EDGES_MAX) return scn_fail(SCN_E_INVALID, "a level table has 1 ... %u edges: %u", SCN_LEVELS_EDGES_MAX, n_edges);
  if ((uint64_t)cells * (n_edges + 1u) > SCN_LEVELS_WORDS_MAX)
    return scn_fail(SCN_E_INVALID, "%u cells of %u levels: more than %u counters", cells, n_edges + 1u, SCN_LEVELS_WORDS_MAX);
  return SCN_OK;
}

int check_levels_edges(const float *edges_db, uint32_t n_edges, uint32_t *keys) {
  if (!edges_db) return scn_fail(SCN_E_INVALID, "null argument");
  if (n_edges == 0 || n_edges > SCN_LEVELS_EDGES_MAX) return scn_fail(SCN_E_INVALID, "a level table has 1 ... %u edges: %u", SCN_LEVELS_EDGES_MAX, n_edges);
  uint32_t below = 0;
  for (uint32_t e = 0; e < n_edges; e++) {
    uint32_t bits;
    memcpy(&bits, edges_db + e, sizeof(bits));
    if (scn_trace_is_nan(bits)) return scn_fail(SCN_E_INVALID, "edge %u is a NaN", e);
    const uint32_t key = scn_trace_key(bits);
    if (e != 0 && key <= below) return scn_fail(SCN_E_INVALID, "edge %u is not above edge %u", e, e - 1u);
    below = key;
  }
  for (uint32_t e = 0; e < kLevelsKeys; e++) {
    uint32_t bits = 0;
    if (e < n_edges) memcpy(&bits, edges_db + e, sizeof(bits));
    keys[e] = e < n_edges ? scn_trace_key(bits) : kLevelsPadKey;
  }
  return SCN_OK;
}

int check_levels_summary(uint32_t n_levels, uint32_t permille, uint32_t level) {
  if (permille > 1000u) return scn_fail(SCN_E_INVALID, "permille %u above 1000", permille);
  if (level >= n_levels) return scn_fail(SCN_E_INVALID, "level %u of a table of %u levels", level, n_levels);
  return SCN_OK;
}

namespace {

// One cell's hold: *max_db becomes the larger of itself and hi, *min_db the smaller of itself and lo, in the key order of
// scn_trace.h; the winning value's bits are stored as they are
void trace_hold(float *max_db, float *min_db, float hi, float lo) {
  uint32_t cur_max, cur_min, bits_hi, bits_lo;
  memcpy(&cur_max, max_db, sizeof(cur_max));
  memcpy(&cur_min, min_db, sizeof(cur_min));
  memcpy(&bits_hi, &hi, sizeof(bits_hi));
  memcpy(&bits_lo, &lo, sizeof(bits_lo));
  if (scn_trace_key(bits_hi) > scn_trace_key(cur_max)) memcpy(max_db, &bits_hi, sizeof(bits_hi));
  if (scn_trace_key(bits_lo) < scn_trace_key(cur_min)) memcpy(min_db, &bits_lo, sizeof(bits_lo));
}

// An ordered host hit list, unit by unit: unit u owns the maximal run of records at the cursor whose seq_id is the unit's
// (unit_seq_ids[u], or u); each(row of the unit, record) for every record.  A record with i >= n, and records left over behind the
// last unit's, are SCN_E_INVALID.
template <class F>
int walk_history_units(uint32_t rows, uint32_t n, uint32_t first, uint32_t n_units, const uint64_t *unit_seq_ids, const scn_hit *hits, uint64_t n_hits,
                       F each) {
  if (!rows || !n) return scn_fail(SCN_E_INVALID, "a history of %u rows of %u bins", rows, n);
  if (!hits && n_hits) return scn_fail(SCN_E_INVALID, "null argument");
  const uint32_t f = first % rows;
  if ((uint64_t)f + n_units > 0xffffffffull) return scn_fail(SCN_E_INVALID, "%u units from row %u", n_units, f);
  uint64_t k = 0;
  for (uint32_t u = 0; u < n_units; u++) {
    const uint64_t id = unit_seq_ids ? unit_seq_ids[u] : (uint64_t)u;
    const uint32_t row = scn_baseline_row(f, u, rows);
    for (; k < n_hits && hits[k].seq_id == id; k++) {
      if (hits[k].i >= n) return scn_fail(SCN_E_INVALID, "record %llu: i = %u outside the %u bins", (unsigned long long)k, hits[k].i, n);
      each(row, hits[k]);
    }
  }
  if (k != n_hits)
    return scn_fail(SCN_E_INVALID, "record %llu (seq_id %llu) belongs to none of the %u units in order", (unsigned long long)k,
                    (unsigned long long)hits[k].seq_id, n_units);
  return SCN_OK;
}

}  // namespace

// Averaged plans: a submit's arguments alone decide whether it can run -- checked before any copy or kernel is queued
int check_average(uint32_t k, bool sweeps, uint32_t nb, const double *fc) {
  if (nb % k) return scn_fail(SCN_E_INVALID, "n_buffers %u is not a multiple of average %u", nb, k);
  if (!fc) return SCN_OK;
  const uint32_t ng = nb / k;
  for (uint32_t g = 0; g < ng; g++) {
    const size_t b0 = sweeps ? g : (size_t)g * k;
    for (uint32_t b = 1; b < k; b++) {
      const size_t bb = sweeps ? g + (size_t)b * ng : (size_t)g * k + b;
      if (!(fc[bb] == fc[b0]))
        return scn_fail(SCN_E_INVALID, "center_freqs differ inside group %u (buffer %zu: %.17g, its first buffer: %.17g)", g, bb, fc[bb],
                        fc[b0]);
    }
  }
  return SCN_OK;
}

// (the arguments were checked by check_average before anything was queued)
uint32_t group_headers(uint32_t k, bool sweeps, uint32_t nb, const double *&fc, const uint64_t *&seq, std::vector<double> &group_fc,
                       std::vector<uint64_t> &group_seq) {
  const uint32_t ng = nb / k;
  auto buffer_of = [&](uint32_t g, uint32_t b) -> size_t { return sweeps ? g + (size_t)b * ng : (size_t)g * k + b; };
  if (fc) {
    group_fc.resize(ng);
    for (uint32_t g = 0; g < ng; g++) group_fc[g] = fc[buffer_of(g, 0)];
    fc = group_fc.data();
  }
  if (seq || !sweeps) {  // (sweeps without seq_ids: group g's first buffer is buffer g, the compaction kernel's default)
    group_seq.resize(ng);
    for (uint32_t g = 0; g < ng; g++) group_seq[g] = seq ? seq[buffer_of(g, 0)] : (uint64_t)buffer_of(g, 0);
    seq = group_seq.data();
  }
  return ng;
}

// What follows the kernel of a submit: the counts (a DMA on the d2h stream: needs no CU -- or nothing, when the kernel stores them
// to pinned memory itself) and, when the caller is known to want records, the ordered list (two small kernels + a DMA on the list
// stream, beside the next launch).  With overlapped slots both follow the kernel on the slot's own stream -- its next kernel is
// two submits away, and fewer streams keep both compute streams on hardware queues of their own (HIP maps streams onto 4 queues
// by default; with a fifth active stream the two compute streams ended up sharing one).
SubmitRoute submit_route(const SubmitShape &in) {
  SubmitRoute r;
  const bool counted = in.hits && in.units != 0;
  r.list_behind = counted && in.list_wanted;  // (an eager submit)
  r.list_forks = r.list_behind && !in.own_stream;
  // The per-buffer counts reach the host either by a DMA behind the kernel or by the kernel's own stores to pinned memory.
  // Both have a price (profiles/r04_experiments.md section 10).  A store over PCIe holds its wave's in-order memory returns up:
  // ~0.4 ns per buffer on the launch (8192 buffers: 73.5 -> 76.7 us; 32768 1024-point buffers: 75 -> 96 us).  A DMA that waits
  // for a kernel or for another DMA starts ~20 us after it (the runtime resolves the dependency on the host): nothing in a
  // steady loop of long launches, but the whole difference for short ones (2048 buffers per launch, three in flight: 25.5
  // -> 19.3 us per step), and fatal when the ordered list's DMA shares the D2H stream with it (two per submit: 92 us per submit
  // on that stream against 73 us of FFT; records read in place, three in flight: 373 .. 403 -> 429 Gsamples/s).  So the kernel
  // stores the counts itself when the launch has few buffers or the list follows eagerly, and a DMA carries them otherwise.
  // (floor and baseline plans take the route of the paths that are not fused: the detect kernel, not the transform, is the submit's last
  //  kernel, and it stores the counts to device memory only -- counts by DMA or scn_hit_total_kernel, a marker event behind it)
  const bool stored = in.fused && (in.direct_counts || in.units <= kStoredCountsUpTo || r.list_behind);
  // Launches of very many small buffers: the total and the trigger flags (a bit per buffer) by themselves -- the counts stay on
  // the GPU, where the list kernels read them: units / 8 bytes cross PCIe instead of 4 units, and a collect walks nothing.  The
  // reduction (scn_hit_total_kernel) runs behind the kernel ON ITS STREAM and stores into pinned memory itself: such a step is bound
  // by the HOST's calls (a 16-point launch of 524288 buffers takes 27 us on the GPU, every HIP call 4 .. 5 us in a torch process),
  // and this way a submit is three of them -- kernel, reduction, event -- where the route over the side stream took six (event,
  // wait, reduction, DMA, event: 72 -> 56 us per step, profiles/r06_experiments.md section 5).  The reduction takes ~6 us of the
  // compute stream per launch; the counts' DMA it replaces runs beside the next launch but costs three more host calls and 4 bytes
  // per buffer of PCIe.  Measured on one box (profiles/r06_total_ab.txt, us per step of the spectrum + hits leg, counts by DMA ->
  // reduction): 524288 x 16 points 56.5 -> 37.1, 262144 x 64: 74.0 -> 51.5, 262144 x 128: 88.1 -> 82.6, but 131072 x 256: 75.0 ->
  // 81.8, 65536 x 512: 75.0 -> 80.9, 32768 x 1024: 74.8 -> 81.9 -- it pays from 2^18 buffers per launch.  (Round 5's form -- the
  // reduction on a side stream behind an event, the flags still by DMA -- paid only from 2^19: profiles/r05_table_ab.txt.)
  // Not when the list forks: this way records no event behind the kernel, and the list stream would wait for none.  Such a submit
  // takes the DMA way of the same plans below the threshold; what that costs at 2^18 units has never been measured.
  const bool reduced = counted && !stored && in.units >= kTotalKernelFrom && !r.list_forks;
  r.counts = !counted ? Counts::None : stored ? Counts::Stored : reduced ? Counts::Reduced : Counts::Dma;
  r.counts_stream = (r.counts == Counts::Dma && !in.own_stream) ? RouteStream::D2H : RouteStream::Slot;
  // ONE event marks the kernel's end for whoever waits for it: the host (`done`, when nothing else follows on the compute
  // stream: counts stored by the kernel, or no counts at all) or the side streams (`kernel_done`); none where everything that
  // follows stays on the slot's stream.  For LARGE launches it is completed by the kernel's own dispatch packet
  // (hipExtLaunchKernel's stopEvent), otherwise by a marker packet behind the kernel.
  // Measured (scripts/stop_event_check.sh, profiles/r02_stop_event.txt), us per step marker -> in-packet: 33.5 M-sample
  // launches 75.6 -> 73.1 (4096-pt cfloat), 77 -> 74.5 (2048-pt), 60.2 -> 59.3 (int16); 67 M samples 144.5 -> 140.8; but
  // 16.8 M samples 44 -> 46..58 and 8.4 M 31 -> 29..56 (erratic: short kernels that carry an event get serialised).
  if (in.units != 0 && !in.own_stream && !reduced) r.end = r.counts_stream == RouteStream::D2H ? KernelEnd::KernelDone : KernelEnd::Done;
  r.end_in_packet = r.end != KernelEnd::None && in.fused && (uint64_t)in.units * in.n >= kPacketEventFrom;
  r.done_behind_counts = r.end != KernelEnd::Done;
  return r;
}

extern "C" {

const char *scn_error_name(int status) {
  switch (status) {
    case SCN_OK: return "SCN_OK";
    case SCN_E_INVALID: return "SCN_E_INVALID";
    case SCN_E_HIP: return "SCN_E_HIP";
    case SCN_E_NOMEM: return "SCN_E_NOMEM";
    case SCN_E_STATE: return "SCN_E_STATE";
    case SCN_E_TRUNCATED: return "SCN_E_TRUNCATED";
    case SCN_E_NO_DEVICE: return "SCN_E_NO_DEVICE";
    case SCN_E_COMM: return "SCN_E_COMM";
    default: return "SCN_E_UNKNOWN";
  }
}

const char *scn_last_error(void) { return g_last_error.c_str(); }

uint32_t scn_abi_version(void) { return SCN_ABI_VERSION; }

int scn_signals_from_hits(const scn_hit *hits, uint64_t n_hits, uint32_t n, uint32_t sample_rate, uint32_t max_gap, scn_signal *signals,
                          uint64_t cap, uint64_t *n_signals) {
  if (!n_signals) return scn_fail(SCN_E_INVALID, "null argument");
  *n_signals = 0;
  if ((!hits && n_hits) || (!signals && cap)) return scn_fail(SCN_E_INVALID, "null argument");
  if (n == 0) return scn_fail(SCN_E_INVALID, "n = 0");
  const uint32_t bin_step = sample_rate / n;  // process.cpp:39 (truncating)
  uint64_t total = 0;
  scn_signal cur = {};
  for (uint64_t k = 0; k < n_hits; k++) {
    const scn_hit &h = hits[k];
    const bool start = k == 0 || h.seq_id != hits[k - 1].seq_id || h.i <= hits[k - 1].i ||  // a new unit
                       (uint64_t)h.i - hits[k - 1].i > (uint64_t)max_gap + 1u;
    if (start) {
      if (k && total <= cap) signals[total - 1] = cur;
      total++;
      cur.seq_id = h.seq_id;
      cur.first_i = cur.peak_i = h.i;
      cur.peak_power_db = h.power_db;
      cur.peak_freq_hz = h.freq_hz;
      cur.n_hits = 0;
    } else if (h.power_db > cur.peak_power_db) {  // (equal powers: the lowest i stays)
      cur.peak_i = h.i;
      cur.peak_power_db = h.power_db;
      cur.peak_freq_hz = h.freq_hz;
    }
    cur.last_i = h.i;
    cur.n_hits++;
    cur.bandwidth_hz = (cur.last_i - cur.first_i + 1u) * bin_step;
  }
  if (total && total <= cap) signals[total - 1] = cur;
  *n_signals = total;
  if (total > cap) return scn_fail(SCN_E_TRUNCATED, "%llu signals, the first %llu returned", (unsigned long long)total, (unsigned long long)cap);
  return SCN_OK;
}

int scn_history_fold_hits(uint32_t *history, uint32_t *visits, uint32_t rows, uint32_t n, uint32_t first, uint32_t n_units,
                          const uint64_t *unit_seq_ids, const scn_hit *hits, uint64_t n_hits) {
  if (!history || !visits) return scn_fail(SCN_E_INVALID, "null argument");
  // the whole list is checked before a word changes: a refused call leaves the history as it was
  if (int st = walk_history_units(rows, n, first, n_units, unit_seq_ids, hits, n_hits, [](uint32_t, const scn_hit &) {})) return st;
  if (int st = check_history_fold(rows, n_units, false, 0)) return st;
  for (uint32_t u = 0; u < n_units; u++) {  // (units <= rows: every unit has a row of its own)
    const uint32_t row = scn_baseline_row(first % rows, u, rows);
    uint32_t *const h = history + (size_t)row * n;
    for (uint32_t i = 0; i < n; i++) h[i] = scn_history_fold(h[i], 0u);
    if (visits[row] != 0xffffffffu) visits[row]++;
  }
  return walk_history_units(rows, n, first, n_units, unit_seq_ids, hits, n_hits,
                            [&](uint32_t row, const scn_hit &r) { history[(size_t)row * n + r.i] |= 1u; });
}

int scn_confirm_hits(const uint32_t *history, uint32_t rows, uint32_t n, uint32_t first, uint32_t n_units, const uint64_t *unit_seq_ids,
                     const scn_hit *hits, uint64_t n_hits, uint32_t m, uint32_t window, scn_hit *out, uint64_t cap, uint64_t *n_out) {
  if (!n_out) return scn_fail(SCN_E_INVALID, "null argument");
  *n_out = 0;
  if (!history || (!out && cap)) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_history_window(m, window)) return st;
  const uint32_t mask = scn_history_mask(window);
  uint64_t total = 0;
  const int st = walk_history_units(rows, n, first, n_units, unit_seq_ids, hits, n_hits, [&](uint32_t row, const scn_hit &r) {
    if (!scn_history_confirms(history[(size_t)row * n + r.i], mask, m)) return;
    if (total < cap) out[total] = r;
    total++;
  });
  if (st) return st;
  *n_out = total;
  if (total > cap) return scn_fail(SCN_E_TRUNCATED, "%llu confirmed records, the first %llu returned", (unsigned long long)total, (unsigned long long)cap);
  return SCN_OK;
}

int scn_trace_init(float *max_db, float *min_db, uint64_t *count, uint32_t cells) {
  if (!max_db || !min_db || !count) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_trace_geometry(1u, cells)) return st;
  const uint32_t below = scn_trace_unkey(kTraceEmptyMaxKey), above = scn_trace_unkey(kTraceEmptyMinKey);  // -inf, +inf
  for (uint32_t c = 0; c < cells; c++) {
    memcpy(max_db + c, &below, sizeof(below));
    memcpy(min_db + c, &above, sizeof(above));
    count[c] = 0;
  }
  return SCN_OK;
}

int scn_trace_merge(float *max_db, float *min_db, uint64_t *count, const float *src_max, const float *src_min, const uint64_t *src_count,
                    uint32_t cells) {
  if (!max_db || !min_db || !count || !src_max || !src_min || !src_count) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_trace_geometry(1u, cells)) return st;
  for (uint32_t c = 0; c < cells; c++) {
    trace_hold(max_db + c, min_db + c, src_max[c], src_min[c]);
    count[c] += src_count[c];
  }
  return SCN_OK;
}

int scn_trace_emitters(const float *max_db, const float *min_db, const uint64_t *count, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells,
                       uint32_t first_cell_index, uint32_t line, float threshold_db, uint32_t max_gap, scn_emitter *out, uint64_t cap, uint64_t *n_emitters) {
  if (!n_emitters) return scn_fail(SCN_E_INVALID, "null argument");
  *n_emitters = 0;
  if (!max_db || !min_db || !count || (!out && cap)) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_trace_geometry(cell_hz, cells)) return st;
  if (int st = check_trace_range(SCN_TRACE_CELLS_MAX, first_cell_index, cells)) return st;
  if (int st = check_emitters_line(line, threshold_db)) return st;
  const uint32_t threshold_bits = scn_emit_bits(threshold_db);
  uint64_t total = 0, peak_key = 0;
  scn_emitter r = {};
  bool open = false;
  // the open emitter's record, closed when the next one starts and behind the last cell
  const auto close = [&]() {
    if (!open) return;
    const uint32_t pc = scn_emit_peak_cell(peak_key), w = pc - first_cell_index;
    uint32_t mx, mn;
    memcpy(&mx, max_db + w, sizeof(mx));
    memcpy(&mn, min_db + w, sizeof(mn));
    r.start_hz = scn_emit_hz(f0_hz, cell_hz, r.first_cell);
    r.stop_hz = scn_emit_hz(f0_hz, cell_hz, (uint64_t)r.last_cell + 1u);
    r.peak_hz = scn_emit_hz(f0_hz, cell_hz, pc);
    r.peak_cell = pc;
    r.peak_db = scn_emit_float(scn_emit_peak_bits(peak_key));
    r.peak_other_db = scn_emit_float(scn_emit_other(line, mx, mn));
    if (total < cap) out[total] = r;
    total++;
  };
  for (uint32_t w = 0; w < cells; w++) {
    uint32_t mx, mn;
    memcpy(&mx, max_db + w, sizeof(mx));
    memcpy(&mn, min_db + w, sizeof(mn));
    const uint32_t v = scn_emit_value(line, mx, mn), c = first_cell_index + w;
    if (!scn_emit_on(count[w], v, threshold_bits)) continue;
    if (scn_emit_starts(open, r.last_cell, c, max_gap)) {
      close();
      r = scn_emitter{};
      r.first_cell = c;
      peak_key = 0;
      open = true;
    }
    r.last_cell = c;
    r.n_cells++;
    r.count += count[w];
    peak_key = std::max(peak_key, scn_emit_peak_key(v, c));
  }
  close();
  *n_emitters = total;
  if (total > cap) return scn_fail(SCN_E_TRUNCATED, "%llu emitters, the first %llu returned", (unsigned long long)total, (unsigned long long)cap);
  return SCN_OK;
}

int scn_trace_fold_spectrum(float *max_db, float *min_db, uint64_t *count, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells, const float *power_db,
                            uint32_t n_units, uint32_t n, uint32_t sample_rate, uint32_t dc_ignore_bins, double use_bandwidth,
                            const double *center_freqs) {
  if (!max_db || !min_db || !count || (n_units && (!power_db || !center_freqs))) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_trace_geometry(cell_hz, cells)) return st;
  if (n == 0 || n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad bin count %u", n);
  if (sample_rate == 0) return scn_fail(SCN_E_INVALID, "sample_rate must be > 0");
  struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore_bins ? dc_ignore_bins : 4u, 0, 0};  // the descriptor's defaults (scn_plan_create)
  if (mask.dc_ignore == SCN_DC_IGNORE_NONE) mask.dc_ignore = 0;
  evaluated_bins(n, mask.dc_ignore, use_bandwidth == 0.0 ? 0.75 : use_bandwidth, &mask.i_lo, &mask.i_hi);
  const uint32_t bin_step = sample_rate / n;  // process.cpp:39 (truncating)
  for (uint32_t u = 0; u < n_units; u++) {
    const double start_frequency = scn_trace_start(center_freqs[u], sample_rate);
    const float *const row = power_db + (size_t)u * n;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t j = (i + n / 2) % n;
      if (!scn_bin_evaluated(j, i, n, mask)) continue;
      uint32_t bits;
      memcpy(&bits, row + j, sizeof(bits));
      if (scn_trace_is_nan(bits)) continue;
      const uint32_t c = scn_trace_cell(scn_trace_freq(start_frequency, i, bin_step), f0_hz, cell_hz, cells);
      if (c == kTraceNoCell) continue;
      trace_hold(max_db + c, min_db + c, row[j], row[j]);
      count[c]++;
    }
  }
  return SCN_OK;
}

int scn_levels_fold_spectrum(uint64_t *hist, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells, const float *edges_db, uint32_t n_edges,
                             const float *power_db, uint32_t n_units, uint32_t n, uint32_t sample_rate, uint32_t dc_ignore_bins, double use_bandwidth,
                             const double *center_freqs) {
  if (!hist || !edges_db || (n_units && (!power_db || !center_freqs))) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = check_levels_geometry(cell_hz, cells, n_edges)) return st;
  uint32_t keys[kLevelsKeys];
  if (int st = check_levels_edges(edges_db, n_edges, keys)) return st;
  if (n == 0 || n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad bin count %u", n);
  if (sample_rate == 0) return scn_fail(SCN_E_INVALID, "sample_rate must be > 0");
  struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore_bins ? dc_ignore_bins : 4u, 0, 0};  // the descriptor's defaults (scn_plan_create)
  if (mask.dc_ignore == SCN_DC_IGNORE_NONE) mask.dc_ignore = 0;
  evaluated_bins(n, mask.dc_ignore, use_bandwidth == 0.0 ? 0.75 : use_bandwidth, &mask.i_lo, &mask.i_hi);
  const uint32_t bin_step = sample_rate / n;  // process.cpp:39 (truncating)
  const uint32_t top = scn_levels_top(n_edges), n_levels = n_edges + 1u;
  for (uint32_t u = 0; u < n_units; u++) {
    const double start_frequency = scn_trace_start(center_freqs[u], sample_rate);
    const float *const row = power_db + (size_t)u * n;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t j = (i + n / 2) % n;
      if (!scn_bin_evaluated(j, i, n, mask)) continue;
      uint32_t bits;
      memcpy(&bits, row + j, sizeof(bits));
      if (scn_trace_is_nan(bits)) continue;
      const uint32_t c = scn_trace_cell(scn_trace_freq(start_frequency, i, bin_step), f0_hz, cell_hz, cells);
      if (c == kTraceNoCell) continue;
      hist[(size_t)c * n_levels + scn_levels_level(keys, top, scn_trace_key(bits))]++;
    }
  }
  return SCN_OK;
}

int scn_levels_merge(uint64_t *hist, const uint64_t *src, uint32_t cells, uint32_t n_levels) {
  if (!hist || !src) return scn_fail(SCN_E_INVALID, "null argument");
  if (n_levels < 2u) return scn_fail(SCN_E_INVALID, "a level table has 1 ... %u edges: %u", SCN_LEVELS_EDGES_MAX, n_levels - 1u);
  if (int st = check_levels_geometry(1u, cells, n_levels - 1u)) return st;
  for (size_t w = 0; w < (size_t)cells * n_levels; w++) hist[w] += src[w];
  return SCN_OK;
}

int scn_levels_summary(const uint64_t *hist, uint32_t cells, uint32_t n_levels, uint32_t permille, uint32_t level, uint32_t *rank_level,
                       uint64_t *above, uint64_t *total) {
  if (!hist) return scn_fail(SCN_E_INVALID, "null argument");
  if (n_levels < 2u) return scn_fail(SCN_E_INVALID, "a level table has 1 ... %u edges: %u", SCN_LEVELS_EDGES_MAX, n_levels - 1u);
  if (int st = check_levels_geometry(1u, cells, n_levels - 1u)) return st;
  if (int st = check_levels_summary(n_levels, permille, level)) return st;
  for (uint32_t c = 0; c < cells; c++) {
    const uint64_t *const row = hist + (size_t)c * n_levels;
    uint64_t sum = 0, from_level = 0;
    for (uint32_t l = 0; l < n_levels; l++) {
      sum += row[l];
      if (l >= level) from_level += row[l];
    }
    uint32_t rank = kLevelsNoRank;
    if (sum != 0) {
      const uint64_t r = scn_levels_rank(sum, permille);
      uint64_t cum = 0;
      for (rank = 0; (cum += row[rank]) <= r; rank++) {}  // (r < sum: it ends inside the row)
    }
    if (rank_level) rank_level[c] = rank;
    if (above) above[c] = from_level;
    if (total) total[c] = sum;
  }
  return SCN_OK;
}

int scn_floor_from_spectrum(const float *power_db, uint32_t n, uint32_t dc_ignore_bins, double use_bandwidth, uint32_t floor_permille,
                            float *floor_db) {
  if (!power_db || !floor_db) return scn_fail(SCN_E_INVALID, "null argument");
  if (n == 0 || n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad bin count %u", n);
  uint32_t permille = 0;
  if (!floor_permille_of(floor_permille, &permille))
    return scn_fail(SCN_E_INVALID, "floor_permille %u: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN", floor_permille);
  if (!dc_ignore_bins) dc_ignore_bins = 4;  // the descriptor's defaults (scn_plan_create)
  if (dc_ignore_bins == SCN_DC_IGNORE_NONE) dc_ignore_bins = 0;
  if (use_bandwidth == 0.0) use_bandwidth = 0.75;
  struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore_bins, 0, 0};
  evaluated_bins(n, dc_ignore_bins, use_bandwidth, &mask.i_lo, &mask.i_hi);
  std::vector<uint32_t> keys;
  keys.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = (i + n / 2) % n;
    if (!scn_bin_evaluated(j, i, n, mask)) continue;
    uint32_t bits;
    memcpy(&bits, power_db + j, sizeof(bits));
    keys.push_back((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));
  }
  if (keys.empty()) return scn_fail(SCN_E_INVALID, "the mask (dc_ignore_bins, use_bandwidth) lets no bin through");
  const size_t r = (size_t)((uint64_t)permille * (keys.size() - 1u) / 1000u);
  std::nth_element(keys.begin(), keys.begin() + (ptrdiff_t)r, keys.end());
  const uint32_t key = keys[r], bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  memcpy(floor_db, &bits, sizeof(bits));
  return SCN_OK;
}

int scn_local_floor_from_spectrum(const float *power_db, uint32_t n, uint32_t dc_ignore_bins, double use_bandwidth, uint32_t floor_permille,
                                  uint32_t train_bins, uint32_t guard_bins, float *floor_db) {
  if (!power_db || !floor_db) return scn_fail(SCN_E_INVALID, "null argument");
  if (n == 0 || n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad bin count %u", n);
  uint32_t permille = 0;
  if (!floor_permille_of(floor_permille, &permille))
    return scn_fail(SCN_E_INVALID, "floor_permille %u: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN", floor_permille);
  struct { uint32_t dc_ignore, i_lo, i_hi; } mask = {dc_ignore_bins ? dc_ignore_bins : 4u, 0, 0};  // the descriptor's defaults (scn_plan_create)
  if (mask.dc_ignore == SCN_DC_IGNORE_NONE) mask.dc_ignore = 0;
  if (!evaluated_bins(n, mask.dc_ignore, use_bandwidth == 0.0 ? 0.75 : use_bandwidth, &mask.i_lo, &mask.i_hi))
    return scn_fail(SCN_E_INVALID, "the mask (dc_ignore_bins, use_bandwidth) lets no bin through");
  if (!train_bins && !guard_bins) {  // no window: the unit-wide floor
    float unit_floor;
    if (int st = scn_floor_from_spectrum(power_db, n, dc_ignore_bins, use_bandwidth, floor_permille, &unit_floor)) return st;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t j = (i + n / 2) % n;
      if (scn_bin_evaluated(j, i, n, mask)) floor_db[j] = unit_floor;
    }
    return SCN_OK;
  }
  std::vector<uint16_t> need;
  if (int st = floor_window_ranks(n, mask.dc_ignore, mask.i_lo, mask.i_hi, permille, train_bins, guard_bins, need)) return st;
  std::vector<uint32_t> keys(n);  // in fftshift order (read before anything is written: floor_db may be power_db)
  for (uint32_t i = 0; i < n; i++) {
    uint32_t bits;
    memcpy(&bits, power_db + (i + n / 2) % n, sizeof(bits));
    keys[i] = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  uint32_t cells[2u * SCN_FLOOR_TRAIN_MAX];
  const int64_t reach = (int64_t)guard_bins + train_bins;
  for (uint32_t i = 0; i < n; i++) {
    if (!need[i]) continue;
    uint32_t m = 0;
    auto take = [&](int64_t lo, int64_t hi) {  // the evaluated bins of [lo, hi], clipped to the band: no wrap
      for (int64_t c = std::max<int64_t>(lo, 0); c <= std::min<int64_t>(hi, (int64_t)n - 1); c++)
        if (need[(size_t)c]) cells[m++] = keys[(size_t)c];
    };
    take((int64_t)i - reach, (int64_t)i - guard_bins - 1);
    take((int64_t)i + guard_bins + 1, (int64_t)i + reach);
    const uint32_t r = need[i] - 1u;  // < m
    std::nth_element(cells, cells + r, cells + m);
    const uint32_t key = cells[r], bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    memcpy(floor_db + (i + n / 2) % n, &bits, sizeof(bits));
  }
  return SCN_OK;
}

int scn_frequency_table(uint32_t sample_rate, double start, double stop, double use_bandwidth,
                        double dc_ignore_width, uint32_t shard, uint32_t n_shards, double *out, uint32_t cap,
                        uint32_t *count, uint32_t *first) {
  if (!count || n_shards == 0 || shard >= n_shards) return scn_fail(SCN_E_INVALID, "bad shard arguments");
  // frequencyTable.cpp:17-29
  double f1 = start + use_bandwidth / 2 * sample_rate;
  double step = use_bandwidth;
  if (dc_ignore_width > 0) step = (use_bandwidth - dc_ignore_width) / 2;
  uint32_t total = 0;
  if (stop == 0.0) {
    total = 1;
  } else {
    if (!(step * (double)sample_rate > 0)) return scn_fail(SCN_E_INVALID, "frequency step must be positive");
    while (f1 + total * step * (double)sample_rate < stop) total++;
  }
  // contiguous index range [lo, hi) of this shard
  uint32_t lo = (uint32_t)((uint64_t)total * shard / n_shards);
  uint32_t hi = (uint32_t)((uint64_t)total * (shard + 1) / n_shards);
  if (first) *first = lo;
  *count = hi - lo;
  if (out)
    for (uint32_t i = lo; i < hi && i - lo < cap; i++) out[i - lo] = f1 + i * step * (double)sample_rate;  // :33
  return SCN_OK;
}

int scn_hackrf_sweep_fixup(void *transfer, uint32_t valid_length, uint32_t scan_offset_hz,
                           double *center_frequency, uint32_t *n_mismatch) {
  if (!transfer || !center_frequency) return scn_fail(SCN_E_INVALID, "null argument");
  if (valid_length < 12) return scn_fail(SCN_E_INVALID, "a sweep transfer holds at least 6 samples");
  uint8_t *head = static_cast<uint8_t *>(transfer);
  const int8_t *samples = static_cast<const int8_t *>(transfer);
  const uint32_t n_samples = valid_length / 2;  // :188
  uint64_t tuned = 0;
  uint32_t mismatches = 0;
  // one pass per 8192-sample block, every pass looking at the head of the transfer (:191-192)
  for (uint32_t first = 0; first < n_samples; first += 8192) {
    if (head[0] != 0x7F || head[1] != 0x7F) continue;
    uint64_t f = 0;
    for (int k = 7; k >= 0; k--) f = (f << 8) | head[2 + k];  // :194-201
    if (tuned != 0 && tuned != f) mismatches++;               // :202-206
    tuned = f;
    int8_t fill_i = (int8_t)head[10], fill_q = (int8_t)head[11];
    if (first > 0) {  // :209-212, int arithmetic, truncating division, narrowed back to int8
      fill_i = (int8_t)((fill_i + samples[2 * (first - 1)]) / 2);
      fill_q = (int8_t)((fill_q + samples[2 * (first - 1) + 1]) / 2);
    }
    for (int j = 0; j < 5; j++) {
      head[2 * j] = (uint8_t)fill_i;
      head[2 * j + 1] = (uint8_t)fill_q;
    }
  }
  *center_frequency = (double)(tuned + scan_offset_hz);  // u64 + u32, then to double (:221)
  if (n_mismatch) *n_mismatch = mismatches;
  return SCN_OK;
}

}  // extern "C"
