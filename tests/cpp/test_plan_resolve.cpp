// What a descriptor resolves to (scanner_amd/csrc/scn_host.hip: resolve_plan, resolve_welch, welch_parts), the size rules of
// scn_sizes.h and the fused kernels' regrouped twiddle tables, as a stand-alone program: built by g++ -x c++ together with that unit,
// no HIP header on the include path, plain and under ASan + UBSan (tests/test_plan_resolve_cpp.py).  Every expected number is written
// out here from the rules of include/scanner_hip.h: for a frequency-domain plan with the default mask, use_window = floor(0.375 n),
// i_lo / i_hi = n/2 -/+ use_window, and the 2 * 4 - 1 bins around DC go, so 2 use_window + 1 - 7 bins are evaluated.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scn_host.h"

static int g_failed = 0;
static unsigned g_descs = 0;  // descriptors put through resolve_plan / resolve_welch
static const char *g_what = "";
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s:%d: %s  (%s)\n", __FILE__, __LINE__, #cond, g_what); \
      g_failed++;                                                                \
    }                                                                            \
  } while (0)

static std::string text(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

static_assert(sizeof(scn_plan_desc) == 88 && sizeof(scn_welch_desc) == 40, "the descriptors have no padding: memcmp compares every field");

// a caller's descriptor with every optional field left at zero ...
static scn_plan_desc given(uint32_t n) {
  scn_plan_desc d = {};
  d.struct_size = sizeof(d);
  d.n = n;
  d.sample_rate = 20000000;
  d.sample_kind = SCN_KIND_FLOAT_COMPLEX;
  d.threshold = -30.0f;
  d.max_batch = 8;
  return d;
}
// ... and what it must come back as
static scn_plan_desc defaulted(uint32_t n) {
  scn_plan_desc d = given(n);
  d.window_type = SCN_WIN_BLACKMAN_HARRIS;
  d.mode = SCN_MODE_FREQUENCY_DOMAIN;
  d.dc_ignore_bins = 4;
  d.use_bandwidth = 0.75;
  d.trigger_count = 1047;
  d.max_hits = 512;
  d.flags = SCN_OUT_SPECTRUM | SCN_OUT_HITS;
  return d;
}

struct Want {
  Path path;
  uint32_t avg, avg_layout;
  size_t buf_bytes;
  float scale;
  uint32_t i_lo, i_hi, hit_region;
  bool floor;
  uint32_t floor_rank, floor_permille;
  bool baseline, direct_counts;
};

static void accept(const char *what, const scn_plan_desc &in, const scn_plan_desc &d, const Want &w) {
  g_what = what;
  g_descs++;
  PlanShape s;
  const int st = resolve_plan(&in, &s);
  CHECK(st == SCN_OK);
  if (st != SCN_OK) {
    std::printf("  refused: %s\n", scn_last_error());
    return;
  }
  CHECK(memcmp(&s.d, &d, sizeof(d)) == 0);
  CHECK(s.d.window_type == d.window_type && s.d.mode == d.mode && s.d.dc_ignore_bins == d.dc_ignore_bins && s.d.use_bandwidth == d.use_bandwidth);
  CHECK(s.d.trigger_count == d.trigger_count && s.d.max_hits == d.max_hits && s.d.flags == d.flags);
  CHECK(s.path == w.path);
  CHECK(s.avg == w.avg && s.avg_layout == w.avg_layout);
  CHECK(s.buf_bytes == w.buf_bytes);
  CHECK(memcmp(&s.scale, &w.scale, sizeof(float)) == 0);
  CHECK(s.i_lo == w.i_lo && s.i_hi == w.i_hi);
  CHECK(s.hit_region == w.hit_region);
  CHECK(s.floor == w.floor && s.floor_rank == w.floor_rank && s.floor_permille == w.floor_permille);
  CHECK(s.baseline == w.baseline);
  CHECK(s.direct_counts == w.direct_counts);
}

static void reject(const char *what, const scn_plan_desc &in, const std::string &message) {
  g_what = what;
  g_descs++;
  PlanShape s;
  const int st = resolve_plan(&in, &s);
  CHECK(st == SCN_E_INVALID);
  if (message != scn_last_error()) std::printf("  got:  %s\n  want: %s\n", scn_last_error(), message.c_str());
  CHECK(message == scn_last_error());
}

static void test_paths_resolved() {
  const uint32_t D = SCN_AVG_DWELL;
  const bool F = false, T = true;
  // one size of each path at its edges, float samples (8 bytes each), the default mask
  accept("16 fused", given(16), defaulted(16), {Path::FusedPow2, 1, D, 128, 1.0f, 2, 14, 6, F, 0, 0, F, F});
  accept("16384 fused", given(16384), defaulted(16384), {Path::FusedPow2, 1, D, 131072, 1.0f, 2048, 14336, 12282, F, 0, 0, F, T});
  accept("8192 fused", given(8192), defaulted(8192), {Path::FusedPow2, 1, D, 65536, 1.0f, 1024, 7168, 6138, F, 0, 0, F, T});
  accept("4096 fused", given(4096), defaulted(4096), {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  accept("1000 mixed", given(1000), defaulted(1000), {Path::FusedMixed, 1, D, 8000, 1.0f, 125, 875, 744, F, 0, 0, F, F});
  accept("10000 mixed", given(10000), defaulted(10000), {Path::FusedMixed, 1, D, 80000, 1.0f, 1250, 8750, 7494, F, 0, 0, F, T});
  accept("16000 mixed", given(16000), defaulted(16000), {Path::FusedMixed, 1, D, 128000, 1.0f, 2000, 14000, 11994, F, 0, 0, F, T});
  // 17: use_window = floor(6.375) = 6 around n/2 = 8; 65535: floor(24575.625) around 32767
  accept("17 Bluestein", given(17), defaulted(17), {Path::Bluestein, 1, D, 136, 1.0f, 2, 14, 6, F, 0, 0, F, F});
  accept("65535 Bluestein", given(65535), defaulted(65535), {Path::Bluestein, 1, D, 524280, 1.0f, 8192, 57342, 49144, F, 0, 0, F, F});
  accept("32768 four-step", given(32768), defaulted(32768), {Path::FourStep, 1, D, 262144, 1.0f, 4096, 28672, 24570, F, 0, 0, F, F});
  accept("65536 four-step", given(65536), defaulted(65536), {Path::FourStep, 1, D, 524288, 1.0f, 8192, 57344, 49146, F, 0, 0, F, F});
  // time-domain mode takes any n >= 1; the mask is computed all the same (100: use_window 37; 1: nothing is left, hit_region stays 1)
  scn_plan_desc in = given(100), out = defaulted(100);
  in.mode = out.mode = SCN_MODE_TIME_DOMAIN;
  accept("time domain 100", in, out, {Path::TimeDomain, 1, D, 800, 1.0f, 13, 87, 68, F, 0, 0, F, F});
  in = given(1), out = defaulted(1);
  in.mode = out.mode = SCN_MODE_TIME_DOMAIN;
  accept("time domain 1", in, out, {Path::TimeDomain, 1, D, 8, 1.0f, 0, 0, 1, F, 0, 0, F, F});
  in = given(8192), out = defaulted(8192);  // (8192 points, but no fused kernel stores its counts)
  in.mode = out.mode = SCN_MODE_TIME_DOMAIN;
  accept("time domain 8192", in, out, {Path::TimeDomain, 1, D, 65536, 1.0f, 1024, 7168, 6138, F, 0, 0, F, F});
}

static void test_defaults_resolved() {
  const uint32_t D = SCN_AVG_DWELL;
  const bool F = false;
  // values the caller gave stay
  scn_plan_desc in = given(4096), out;
  in.window_type = SCN_WIN_HANN;
  in.mode = SCN_MODE_FREQUENCY_DOMAIN;
  in.dc_ignore_bins = 10;
  in.use_bandwidth = 0.5;
  in.trigger_count = 3;
  in.max_hits = 77;
  in.flags = SCN_OUT_HITS;
  in.correct_dc = 1;
  in.device_id = 5;  // (not resolve_plan's to check)
  out = in;
  // use_window 1024: [1024, 3072], 2049 bins less the 19 around DC
  accept("nothing defaulted", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 1024, 3072, 2030, F, 0, 0, F, F});
  // the flags: neither output means both, whatever else is set; one output stays alone
  in = given(4096), out = defaulted(4096);
  in.flags = SCN_PLAN_OVERLAP_SLOTS;
  out.flags = SCN_PLAN_OVERLAP_SLOTS | SCN_OUT_SPECTRUM | SCN_OUT_HITS;
  accept("flags: overlap alone", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.flags = out.flags = SCN_OUT_SPECTRUM;
  accept("flags: spectrum alone", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  // max_hits 0: 64 per buffer, at most 2^28
  in = given(4096), out = defaulted(4096);
  in.max_batch = out.max_batch = 1;
  out.max_hits = 64;
  accept("max_hits of 1 buffer", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.max_batch = out.max_batch = 1u << 22;
  out.max_hits = 1u << 28;
  accept("max_hits at the cap", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.max_batch = out.max_batch = (1u << 22) + 1u;
  accept("max_hits past the cap", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.max_batch = out.max_batch = 0xffffffffu;  // (64 times it does not fit 32 bits)
  accept("max_hits of 2^32 - 1 buffers", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  // the DC window: 0 is 4, SCN_DC_IGNORE_NONE is none (all 2 * 1536 + 1 bins of the band)
  in = given(4096), out = defaulted(4096);
  in.dc_ignore_bins = SCN_DC_IGNORE_NONE;
  out.dc_ignore_bins = 0;
  accept("no DC window", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3073, F, 0, 0, F, F});
  // use_bandwidth 0.001: use_window = floor(2.048) = 2, i in [2046, 2050] = j in {4094, 4095, 0, 1, 2}, all within 3 of DC
  in.dc_ignore_bins = out.dc_ignore_bins = 3;
  in.use_bandwidth = out.use_bandwidth = 0.001;
  accept("a mask that leaves no bin", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 2046, 2050, 1, F, 0, 0, F, F});
  in.dc_ignore_bins = out.dc_ignore_bins = 2;  // ... and j = 4094, 2 with a window of 2
  accept("a mask that leaves two bins", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 2046, 2050, 2, F, 0, 0, F, F});
}

static void test_formats_resolved() {
  const uint32_t D = SCN_AVG_DWELL;
  const bool F = false;
  scn_plan_desc in = given(4096), out = defaulted(4096);
  in.sample_kind = out.sample_kind = SCN_KIND_BYTE_COMPLEX;
  in.enob = out.enob = 7;
  accept("int8, 7 bits", in, out, {Path::FusedPow2, 1, D, 8192, 1.0f / 64.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.enob = out.enob = 8;  // (the reference's narrowing wrap: int8_t(128) = -128)
  accept("int8, 8 bits", in, out, {Path::FusedPow2, 1, D, 8192, -1.0f / 128.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.sample_kind = out.sample_kind = SCN_KIND_SHORT;
  in.enob = out.enob = 12;
  accept("int16 planar, 12 bits", in, out, {Path::FusedPow2, 1, D, 16384, 1.0f / 2048.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.sample_kind = out.sample_kind = SCN_KIND_SHORT_COMPLEX;
  accept("int16, 12 bits", in, out, {Path::FusedPow2, 1, D, 16384, 1.0f / 2048.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in.enob = out.enob = 16;
  accept("int16, 16 bits", in, out, {Path::FusedPow2, 1, D, 16384, -1.0f / 32768.0f, 512, 3584, 3066, F, 0, 0, F, F});
  in = given(4096), out = defaulted(4096);
  in.enob = out.enob = 0;  // float samples: enob is not read
  accept("float", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
}

static void test_average_resolved() {
  const uint32_t D = SCN_AVG_DWELL, S = SCN_AVG_SWEEPS;
  const bool F = false, T = true;
  // 1024 points: use_window 384, [128, 896], 769 - 7 bins
  scn_plan_desc in = given(1024), out = defaulted(1024);
  in.average = out.average = 4;
  accept("average 4, dwell", in, out, {Path::FusedPow2, 4, D, 8192, 1.0f, 128, 896, 762, F, 0, 0, F, F});
  in.average_layout = out.average_layout = S;
  accept("average 4, sweeps", in, out, {Path::FusedPow2, 4, S, 8192, 1.0f, 128, 896, 762, F, 0, 0, F, F});
  // average 1 (given, or 0): the layout is SCN_AVG_DWELL whatever the descriptor says, and is not checked
  in.average = out.average = 1;
  accept("average 1, sweeps asked", in, out, {Path::FusedPow2, 1, D, 8192, 1.0f, 128, 896, 762, F, 0, 0, F, F});
  in.average = out.average = 0;
  in.average_layout = out.average_layout = 7;
  accept("average 0, unknown layout", in, out, {Path::FusedPow2, 1, D, 8192, 1.0f, 128, 896, 762, F, 0, 0, F, F});
  in.average_layout = out.average_layout = D;
  in.average = out.average = 1;
  accept("average 1, dwell", in, out, {Path::FusedPow2, 1, D, 8192, 1.0f, 128, 896, 762, F, 0, 0, F, F});
  in = given(8192), out = defaulted(8192);
  in.average = out.average = 8;
  accept("average 8 at 8192", in, out, {Path::FusedPow2, 8, D, 65536, 1.0f, 1024, 7168, 6138, F, 0, 0, F, T});
}

static void test_detect_resolved() {
  const uint32_t D = SCN_AVG_DWELL;
  const bool F = false, T = true;
  scn_plan_desc in = given(4096), out = defaulted(4096);
  in.detect = out.detect = SCN_DETECT_FIXED;
  in.floor_permille = out.floor_permille = 5000;  // (not read outside floor mode)
  accept("fixed", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, F, F});
  // floor: rank = permille * 3065 / 1000, truncating
  in = given(4096), out = defaulted(4096);
  in.detect = out.detect = SCN_DETECT_FLOOR;
  accept("floor, the median", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, T, 1532, 500, F, F});
  in.floor_permille = out.floor_permille = 1;
  accept("floor, permille 1", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, T, 3, 1, F, F});
  in.floor_permille = out.floor_permille = 1000;
  accept("floor, the maximum", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, T, 3065, 1000, F, F});
  in.floor_permille = out.floor_permille = SCN_FLOOR_MIN;
  accept("floor, the minimum", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, T, 0, 0, F, F});
  in = given(65536), out = defaulted(65536);  // the largest rank a plan can have: 49145
  in.detect = out.detect = SCN_DETECT_FLOOR;
  in.floor_permille = out.floor_permille = 1000;
  in.flags = out.flags = SCN_OUT_HITS;
  accept("floor, 65536 points", in, out, {Path::FourStep, 1, D, 524288, 1.0f, 8192, 57344, 49146, T, 49145, 1000, F, F});
  in = given(4096), out = defaulted(4096);  // one evaluated bin would do: two here (see the mask above), rank 1 * 1 / 1000 ... 1000 * 1 / 1000
  in.detect = out.detect = SCN_DETECT_FLOOR;
  in.dc_ignore_bins = out.dc_ignore_bins = 2;
  in.use_bandwidth = out.use_bandwidth = 0.001;
  in.floor_permille = out.floor_permille = 999;
  accept("floor over two bins, permille 999", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 2046, 2050, 2, T, 0, 999, F, F});
  in.floor_permille = out.floor_permille = 1000;
  accept("floor over two bins, the maximum", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 2046, 2050, 2, T, 1, 1000, F, F});
  // baseline: the caller's own flags must name SCN_OUT_HITS
  in = given(4096), out = defaulted(4096);
  in.detect = out.detect = SCN_DETECT_BASELINE;
  in.flags = out.flags = SCN_OUT_HITS;
  accept("baseline, hits", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, T, F});
  in.flags = out.flags = SCN_OUT_HITS | SCN_OUT_SPECTRUM;
  in.floor_permille = out.floor_permille = 5000;  // (not read)
  accept("baseline, both outputs", in, out, {Path::FusedPow2, 1, D, 32768, 1.0f, 512, 3584, 3066, F, 0, 0, T, F});
  in = given(8192), out = defaulted(8192);
  in.detect = out.detect = SCN_DETECT_BASELINE;
  in.flags = out.flags = SCN_OUT_HITS;
  in.average = out.average = 2;
  accept("baseline, averaged, 8192", in, out, {Path::FusedPow2, 2, D, 65536, 1.0f, 1024, 7168, 6138, F, 0, 0, T, T});
}

// every rejection alone, then with the check behind it failing too: the earlier one wins
static void test_rejections() {
  scn_plan_desc d = given(4096);
  d.struct_size = 84;
  reject("struct_size", d, text("scn_plan_desc.struct_size %u != %zu (ABI mismatch)", 84u, (size_t)88));
  d.max_batch = 0;
  reject("struct_size before max_batch", d, "scn_plan_desc.struct_size 84 != 88 (ABI mismatch)");
  d = given(4096);
  d.max_batch = 0;
  reject("max_batch", d, "max_batch must be >= 1");
  d.sample_kind = 9;
  reject("max_batch before sample_kind", d, "max_batch must be >= 1");
  d = given(4096);
  d.sample_kind = 0;
  reject("sample_kind 0", d, "unknown sample_kind 0");
  d.sample_kind = 5;
  reject("sample_kind 5", d, "unknown sample_kind 5");
  d.sample_kind = 9;
  d.enob = 40;
  reject("sample_kind before enob", d, "unknown sample_kind 9");
  d = given(4096);
  d.sample_kind = SCN_KIND_SHORT_COMPLEX;
  reject("enob 0", d, "enob 0 out of range");
  d.enob = 33;
  reject("enob 33", d, "enob 33 out of range");
  d.window_type = 9;
  reject("enob before window_type", d, "enob 33 out of range");
  d = given(4096);
  d.window_type = 9;
  reject("window_type", d, "unsupported window_type 9");
  d.mode = 3;
  reject("window_type before mode", d, "unsupported window_type 9");
  d = given(4096);
  d.mode = 3;
  reject("mode", d, "unsupported mode 3");
  d.n = 8;
  reject("mode before size", d, "unsupported mode 3");
  d = given(15);
  reject("size 15", d, "unsupported FFT size 15 (16 to 65536)");
  d.n = 65537;
  reject("size 65537", d, "unsupported FFT size 65537 (16 to 65536)");
  d.n = 131072;
  reject("size 2^17", d, "unsupported FFT size 131072 (16 to 65536)");
  d.sample_rate = 0;
  reject("size before sample_rate", d, "unsupported FFT size 131072 (16 to 65536)");
  // frequency-domain mode never reaches the sample-count check: the size check has refused both of its cases
  d = given(0);
  reject("size 0, frequency domain", d, "unsupported FFT size 0 (16 to 65536)");
  d.n = (1u << 24) + 1u;
  reject("size 2^24 + 1, frequency domain", d, "unsupported FFT size 16777217 (16 to 65536)");
  d.mode = SCN_MODE_TIME_DOMAIN;
  reject("sample count 2^24 + 1", d, "bad sample count 16777217");
  d.n = 0;
  reject("sample count 0", d, "bad sample count 0");
  d.sample_rate = 0;
  reject("sample count before sample_rate", d, "bad sample count 0");
  d = given(4096);
  d.sample_rate = 0;
  reject("sample_rate", d, "sample_rate must be > 0");
  d.mode = SCN_MODE_TIME_DOMAIN;
  d.average = 2;
  reject("sample_rate before average", d, "sample_rate must be > 0");

  // the average's checks, in their order, ahead of the detector's
  d = given(4096);
  d.mode = SCN_MODE_TIME_DOMAIN;
  d.average = 2;
  reject("average, time domain", d, "average 2 needs a frequency-domain plan");
  d.n = 100;
  reject("average: time domain before size", d, "average 2 needs a frequency-domain plan");
  d = given(512);
  d.average = 2;
  reject("average, size", d, "average 2: n = 512 is not supported (1024, 2048, 4096, 8192)");
  d.n = 16384;
  d.average = 3;
  reject("average: size before max_batch", d, "average 3: n = 16384 is not supported (1024, 2048, 4096, 8192)");
  d = given(4096);
  d.average = 3;
  reject("average, max_batch", d, "average 3 does not divide max_batch 8");
  d.average_layout = 2;
  reject("average: max_batch before layout", d, "average 3 does not divide max_batch 8");
  d.average = 4;
  reject("average, layout", d, "unknown average_layout 2");
  d.detect = 3;
  reject("average before detect", d, "unknown average_layout 2");
  d.detect = SCN_DETECT_FLOOR;
  d.floor_permille = 1001;
  reject("average before floor", d, "unknown average_layout 2");
  d = given(4096);
  d.average = 3;
  d.detect = SCN_DETECT_BASELINE;
  reject("average before baseline", d, "average 3 does not divide max_batch 8");

  d = given(4096);
  d.detect = 3;
  reject("detect", d, "unknown detect 3");
  // baseline: the mode, then the CALLER's flags -- 0 is refused although the default has by then set both outputs
  d.detect = SCN_DETECT_BASELINE;
  reject("baseline, flags 0", d, "detect = SCN_DETECT_BASELINE needs SCN_OUT_HITS set in flags");
  d.flags = SCN_OUT_SPECTRUM;
  reject("baseline, spectrum only", d, "detect = SCN_DETECT_BASELINE needs SCN_OUT_HITS set in flags");
  d.flags = SCN_PLAN_OVERLAP_SLOTS;
  reject("baseline, overlap only", d, "detect = SCN_DETECT_BASELINE needs SCN_OUT_HITS set in flags");
  d.flags = SCN_OUT_HITS;
  d.mode = SCN_MODE_TIME_DOMAIN;
  reject("baseline, time domain", d, "detect = SCN_DETECT_BASELINE needs a frequency-domain plan");
  d.flags = 0;
  reject("baseline: mode before flags", d, "detect = SCN_DETECT_BASELINE needs a frequency-domain plan");
  // floor: the mode, the flags WITH the default applied (0 is fine, test_detect_resolved), the rank, the mask
  d = given(4096);
  d.detect = SCN_DETECT_FLOOR;
  d.mode = SCN_MODE_TIME_DOMAIN;
  reject("floor, time domain", d, "detect = SCN_DETECT_FLOOR needs a frequency-domain plan");
  d.flags = SCN_OUT_SPECTRUM;
  reject("floor: mode before flags", d, "detect = SCN_DETECT_FLOOR needs a frequency-domain plan");
  d.mode = 0;
  reject("floor, spectrum only", d, "detect = SCN_DETECT_FLOOR needs SCN_OUT_HITS");
  d.floor_permille = 1001;
  reject("floor: flags before permille", d, "detect = SCN_DETECT_FLOOR needs SCN_OUT_HITS");
  d.flags = 0;
  reject("floor, permille 1001", d, "floor_permille 1001: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN");
  d.floor_permille = 0xfffffffeu;
  reject("floor, permille 2^32 - 2", d, "floor_permille 4294967294: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN");
  d.dc_ignore_bins = 3;
  d.use_bandwidth = 0.001;
  reject("floor: permille before mask", d, "floor_permille 4294967294: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN");
  d.floor_permille = 0;
  reject("floor, no bin", d, "detect = SCN_DETECT_FLOOR: the mask (dc_ignore_bins, use_bandwidth) lets no bin through");
}

// the rule test_capi_cpu.py::test_size_paths states, over the same range
#define MIXED_IS(N, ...) || n == N
static Path rule(uint32_t n) {
  const bool pow2 = n > 0 && (n & (n - 1)) == 0;
  const bool mixed = false SCN_MIXED_PLANS(MIXED_IS) SCN_MIXED_BIG_PLANS(MIXED_IS);
  if (pow2 && n >= 16 && n <= 16384) return Path::FusedPow2;
  if (mixed) return Path::FusedMixed;
  if (n == 32768 || n == 65536) return Path::FourStep;
  return n >= 16 && n <= 65535 && !pow2 ? Path::Bluestein : Path::Unsupported;
}

static void test_path_rule() {
  g_what = "path rule";
  uint32_t fused = 0, mixed = 0, four = 0, blue = 0;
  for (uint32_t n = 0; n <= 70000; n++) {
    const Path p = path_of(SCN_MODE_FREQUENCY_DOMAIN, n);
    if (p != rule(n)) std::printf("  n = %u\n", n);
    CHECK(p == rule(n));
    CHECK(path_of(SCN_MODE_TIME_DOMAIN, n) == Path::TimeDomain);
    fused += p == Path::FusedPow2, mixed += p == Path::FusedMixed, four += p == Path::FourStep, blue += p == Path::Bluestein;
    CHECK(scn_avg_size_supported(n) == (n == 1024 || n == 2048 || n == 4096 || n == 8192));
  }
  // 11 powers of two, the 34 sizes of scn_mixed_plans.h, two four-step sizes; 65520 sizes in [16, 65535] less 45 fused and 32768
  CHECK(fused == 11 && mixed == 34 && four == 2 && blue == 65520 - 46);
}

// rows + 1 is the radix of the first pass, one row per non-trivial power; a row holds one entry per pass-1 thread, n / radix
static void test_table_shapes() {
  g_what = "table shapes";
  for (uint32_t n = 16; n <= 16384; n *= 2) {
    uint32_t rows = 0, threads = 0;
    scn_tw1_layout(n, &rows, &threads);
    CHECK(rows == (n == 16384 ? 31u : 15u) && threads == n / (n == 16384 ? 32u : 16u));
    CHECK(!scn_mixed_layout(n, &rows, &threads));
  }
#define MIXED_SHAPE(N, R1, R2, R3, ...)                                     \
  {                                                                         \
    uint32_t rows = 0, threads = 0;                                         \
    CHECK(scn_mixed_layout(N, &rows, &threads));                            \
    CHECK(R1 * R2 * R3 == N && rows == R1 - 1u && threads == N / R1);       \
    CHECK(scn_mixed_size_supported(N) && !scn_fft_size_supported(N));       \
  }
  SCN_MIXED_PLANS(MIXED_SHAPE)
  SCN_MIXED_BIG_PLANS(MIXED_SHAPE)
  uint32_t rows = 7, threads = 9;
  CHECK(!scn_mixed_layout(1001, &rows, &threads) && rows == 7 && threads == 9);
}

static void test_tables() {
  g_what = "fused tables";
  for (uint32_t n : {16u, 128u, 512u, 4096u, 8192u, 16384u, 1000u, 6000u, 16000u}) {
    uint32_t rows = 0, threads = 0;
    if (!scn_mixed_layout(n, &rows, &threads)) scn_tw1_layout(n, &rows, &threads);
    const std::vector<float> tw = twiddles<float>(n), tw1 = fused_tw1_table(n, rows, threads);
    CHECK(tw1.size() == 2 * (size_t)rows * threads);
    if (tw1.size() != 2 * (size_t)rows * threads) continue;
    unsigned bad = 0;
    for (uint32_t p = 1; p <= rows; p++)
      for (uint32_t t = 0; t < threads; t++)
        bad += memcmp(&tw1[2 * ((size_t)(p - 1) * threads + t)], &tw[2 * (size_t)(((uint64_t)t * p) % n)], 2 * sizeof(float)) != 0;
    if (bad) std::printf("  n = %u: %u entries differ\n", n, bad);
    CHECK(bad == 0);
  }
  g_what = "averaged half tables";
  const ScnAvgHalfTables h = avg_half_tables();
  const std::vector<float> tw = twiddles<float>(8192);
  const std::vector<double> twd = twiddles<double>(8192);
  CHECK(h.half.size() == 2 * 15 * 256 && h.join.size() == 2 * 4096);
  if (h.half.size() != 2 * 15 * 256 || h.join.size() != 2 * 4096) return;
  unsigned bad = 0;
  for (uint32_t p = 1; p <= 15; p++)
    for (uint32_t t = 0; t < 256; t++) bad += memcmp(&h.half[2 * ((p - 1) * 256 + t)], &tw[2 * ((2 * t * p) % 8192)], 2 * sizeof(float)) != 0;
  CHECK(bad == 0);
  CHECK(memcmp(h.join.data(), twd.data(), 2 * 4096 * sizeof(double)) == 0);
}

static scn_welch_desc welch_given() {
  scn_welch_desc d = {};
  d.struct_size = sizeof(d);
  d.n = 65536;
  d.segments_per_psd = 3;
  d.max_psd = 2;
  return d;
}

static void welch_accept(const char *what, const scn_welch_desc &in, const scn_welch_desc &d, uint32_t bytes, float scale, bool dc) {
  g_what = what;
  g_descs++;
  WelchShape s;
  const int st = resolve_welch(&in, &s);
  CHECK(st == SCN_OK);
  if (st != SCN_OK) return;
  CHECK(memcmp(&s.d, &d, sizeof(d)) == 0);
  CHECK(s.hop == 32768 && s.bytes_per_sample == bytes && memcmp(&s.scale, &scale, sizeof(float)) == 0 && s.dc == dc);
}

static void welch_reject(const char *what, const scn_welch_desc &in, const std::string &message) {
  g_what = what;
  g_descs++;
  WelchShape s;
  CHECK(resolve_welch(&in, &s) == SCN_E_INVALID);
  if (message != scn_last_error()) std::printf("  got:  %s\n  want: %s\n", scn_last_error(), message.c_str());
  CHECK(message == scn_last_error());
}

static void test_welch() {
  // zeros mean float samples, Blackman-Harris; enob's default is written even where it is not read
  scn_welch_desc in = welch_given(), out = in;
  out.window_type = SCN_WIN_BLACKMAN_HARRIS;
  out.sample_kind = SCN_KIND_FLOAT_COMPLEX;
  out.enob = 12;
  welch_accept("welch, all defaults", in, out, 8, 1.0f, false);
  in.correct_dc = out.correct_dc = 1;  // ignored for float samples
  in.sample_kind = SCN_KIND_FLOAT_COMPLEX;
  in.window_type = out.window_type = SCN_WIN_HAMMING;
  in.enob = out.enob = 99;
  welch_accept("welch, float with correct_dc", in, out, 8, 1.0f, false);
  in = welch_given(), out = in;
  out.window_type = SCN_WIN_BLACKMAN_HARRIS;
  in.sample_kind = out.sample_kind = SCN_KIND_BYTE_COMPLEX;
  out.enob = 8;
  welch_accept("welch, int8", in, out, 2, -1.0f / 128.0f, false);
  in.correct_dc = out.correct_dc = 7;
  in.enob = out.enob = 7;
  welch_accept("welch, int8, 7 bits, correct_dc", in, out, 2, 1.0f / 64.0f, true);
  in = welch_given(), out = in;
  out.window_type = SCN_WIN_BLACKMAN_HARRIS;
  in.sample_kind = out.sample_kind = SCN_KIND_SHORT;
  out.enob = 12;
  welch_accept("welch, int16 planar", in, out, 4, 1.0f / 2048.0f, false);
  in.sample_kind = out.sample_kind = SCN_KIND_SHORT_COMPLEX;
  in.correct_dc = out.correct_dc = 1;
  in.enob = out.enob = 16;
  welch_accept("welch, int16, 16 bits, correct_dc", in, out, 4, -1.0f / 32768.0f, true);

  scn_welch_desc d = welch_given();
  d.struct_size = 36;
  welch_reject("welch struct_size", d, "scn_welch_desc.struct_size mismatch");
  d.sample_kind = 5;
  welch_reject("welch struct_size before sample_kind", d, "scn_welch_desc.struct_size mismatch");
  d = welch_given();
  d.sample_kind = 5;
  welch_reject("welch sample_kind", d, "unsupported sample_kind 5");
  d.enob = 40;
  d.n = 4096;
  welch_reject("welch sample_kind before the rest", d, "unsupported sample_kind 5");
  d = welch_given();
  d.sample_kind = SCN_KIND_BYTE_COMPLEX;
  d.enob = 9;
  welch_reject("welch enob, int8", d, "enob 9 out of range for sample_kind 1");
  d.sample_kind = SCN_KIND_SHORT;
  d.enob = 17;
  welch_reject("welch enob, int16", d, "enob 17 out of range for sample_kind 2");
  d.n = 32768;
  welch_reject("welch enob before n", d, "enob 17 out of range for sample_kind 2");
  d = welch_given();
  d.n = 32768;
  welch_reject("welch n", d, "unsupported Welch segment length 32768 (65536)");
  d.max_psd = 0;
  welch_reject("welch n before max_psd", d, "unsupported Welch segment length 32768 (65536)");
  d = welch_given();
  d.max_psd = 0;
  welch_reject("welch max_psd", d, "segments_per_psd and max_psd must be >= 1");
  d = welch_given();
  d.segments_per_psd = 0;
  welch_reject("welch segments_per_psd", d, "segments_per_psd and max_psd must be >= 1");
  d.window_type = 9;
  welch_reject("welch segments before window_type", d, "segments_per_psd and max_psd must be >= 1");
  d = welch_given();
  d.window_type = 9;
  welch_reject("welch window_type", d, "unsupported window_type 9");

  // the split of a PSD's K segments: doubled while it stays <= 4 and <= K and 16 tiles x max_psd x parts leave CUs idle
  g_what = "welch_parts";
  for (uint32_t max_psd : {1u, 2u, 8u, 16u})
    for (uint32_t k : {1u, 2u, 3u, 16u}) {
      uint32_t parts = 1;
      while (parts < 4 && parts * 2 <= k && 16 * max_psd * parts < 256) parts *= 2;
      CHECK(welch_parts(max_psd, k, 256) == parts);
    }
  CHECK(welch_parts(1, 16, 256) == 4 && welch_parts(8, 16, 256) == 2 && welch_parts(16, 16, 256) == 1 && welch_parts(1, 3, 256) == 2 && welch_parts(1, 1, 256) == 1);
}

int main() {
  test_paths_resolved();
  test_defaults_resolved();
  test_formats_resolved();
  test_average_resolved();
  test_detect_resolved();
  test_rejections();
  test_path_rule();
  test_table_shapes();
  test_tables();
  test_welch();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("plan resolve tests ok (%u descriptors)\n", g_descs);
  return 0;
}
