// K1's decode (scanner_amd/csrc/scn_wire.h) as a stand-alone program: Wire<KIND>::conv / ints / scn_wire_bytes against the oracle's
// conversions (oracle/scn_oracle.c), BIT FOR BIT, over every int16 value and every int8 pair, with DC removal off and on.  Built
// by g++ -x c++, no HIP header on the include path, plain and under ASan + UBSan (tests/test_host_cpp.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scn_host.h"  // convert_scale
#include "scn_oracle.h"
#include "scn_wire.h"

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// the integer formats' register forms, as the loaders build them
static int pack16(int16_t re, int16_t im) { return (int)((uint32_t)(uint16_t)re | ((uint32_t)(uint16_t)im << 16)); }
static int pack8(int8_t re, int8_t im) { return (int)((uint32_t)(uint8_t)re | ((uint32_t)(uint8_t)im << 8)); }

// One buffer (I[n], Q[n]) through the oracle's converter of `kind` and through Wire<KIND>, sample by sample.  With correct_dc
// the test forms the reference's int32 /= uint32 quotient itself (utility.cpp:77-78) from the buffer's integer sums.
template <int KIND, class T>
static void check_buffer(const std::vector<T> &re, const std::vector<T> &im, uint32_t enob, bool correct_dc) {
  typedef Wire<KIND> W;
  const uint32_t n = (uint32_t)re.size();
  std::vector<float> want(2 * (size_t)n);
  if constexpr (KIND == SCN_K_SHORT) {
    scn_oracle_short_planar_to_float_complex((const int16_t *)re.data(), (const int16_t *)im.data(), want.data(), n, enob, correct_dc);
  } else {
    std::vector<T> iq(2 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) iq[2 * i] = re[i], iq[2 * i + 1] = im[i];
    if constexpr (KIND == SCN_K_SHORT_COMPLEX) scn_oracle_short_complex_to_float_complex((const int16_t *)iq.data(), want.data(), n, enob, correct_dc);
    else scn_oracle_byte_complex_to_float_complex((const int8_t *)iq.data(), want.data(), n, enob, correct_dc);
  }
  uint32_t sr = 0, si = 0;  // int32 sums that wrap
  for (uint32_t i = 0; i < n; i++) sr += (uint32_t)(int32_t)re[i], si += (uint32_t)(int32_t)im[i];
  const int dc_re = correct_dc ? (int)(sr / n) : 0, dc_im = correct_dc ? (int)(si / n) : 0;
  const float scale = convert_scale(KIND, enob);
  for (uint32_t i = 0; i < n; i++) {
    const int raw = sizeof(T) == 2 ? pack16((int16_t)re[i], (int16_t)im[i]) : pack8((int8_t)re[i], (int8_t)im[i]);
    int a, b;
    W::ints(raw, a, b);
    CHECK(a == (int)re[i] && b == (int)im[i]);  // the plain C sign extension
    const cf got = W::conv(raw, dc_re, dc_im, scale), unscaled = W::conv(raw, dc_re, dc_im);
    CHECK(bits(got.x) == bits(want[2 * i]) && bits(got.y) == bits(want[2 * i + 1]));
    CHECK(bits(unscaled.x * scale) == bits(got.x) && bits(unscaled.y * scale) == bits(got.y));
  }
}

// `pad` more samples bring the plane's integer sum to `want`
template <class T>
static void pad_to_sum(std::vector<T> &v, uint32_t pad, long want, long top) {
  long rest = want;
  for (T x : v) rest -= x;
  for (uint32_t i = 0; i < pad; i++) {
    const long step = rest > top ? top : rest < -top ? -top : rest;
    v.push_back((T)step);
    rest -= step;
  }
  CHECK(rest == 0);
}

// DC removal off, then on with `pad` samples behind the given ones that make the integer sums over all n negative, zero, n - 1,
// n and n + 1 (I and Q on different ones): the quotients 2^32 / n - 1, 0, 0, 1, 1
template <int KIND, class T>
static void check_format(const std::vector<T> &re0, const std::vector<T> &im0, uint32_t pad, uint32_t enob, long top) {
  check_buffer<KIND>(re0, im0, enob, false);
  const long n = (long)re0.size() + pad, target[5] = {-5, 0, n - 1, n, n + 1};
  for (int which = 0; which < 5; which++) {
    std::vector<T> re = re0, im = im0;
    pad_to_sum(re, pad, target[which], top);
    pad_to_sum(im, pad, target[(which + 2) % 5], top);
    check_buffer<KIND>(re, im, enob, true);
  }
}

static void test_int16() {
  std::vector<int16_t> re(65536), im(65536);
  for (uint32_t i = 0; i < 65536; i++) re[i] = (int16_t)(uint16_t)i, im[i] = (int16_t)(uint16_t)(i * 40503u + 12345u);  // odd multiplier: a permutation
  for (uint32_t enob : {1u, 12u, 14u, 16u}) {
    check_format<SCN_K_SHORT_COMPLEX>(re, im, 8, enob, 32767);
    check_format<SCN_K_SHORT>(re, im, 8, enob, 32767);
  }
  // short buffers: a negative sum over n = 1, 2, 3 gives a quotient near 2^32 / n, and source - dc wraps
  for (uint32_t n = 1; n <= 3; n++) {
    std::vector<int16_t> a(n, (int16_t)-32768), b(n, (int16_t)32767);
    b[0] = (int16_t)(-32767 * (int)(n - 1) - 3);  // sum -3
    check_buffer<SCN_K_SHORT_COMPLEX>(a, b, 12, true);
    check_buffer<SCN_K_SHORT>(b, a, 16, true);
  }
}

static void test_int8() {
  std::vector<int8_t> re(65536), im(65536);
  for (uint32_t i = 0; i < 65536; i++) re[i] = (int8_t)(uint8_t)(i & 255u), im[i] = (int8_t)(uint8_t)(i >> 8);  // every I/Q pair
  check_format<SCN_K_BYTE_COMPLEX>(re, im, 1024, 8, 127);
  for (uint32_t n = 1; n <= 3; n++) {
    std::vector<int8_t> a(n, (int8_t)-128), b(n, (int8_t)127);
    b[0] = (int8_t)(n == 1 ? -3 : n == 2 ? -128 : -128);  // sums -3, -1, 126
    check_buffer<SCN_K_BYTE_COMPLEX>(a, b, 8, true);
  }
}

static void test_float() {
  typedef Wire<SCN_K_FLOAT_COMPLEX> W;
  const uint32_t pat[] = {0x00000000u, 0x80000000u, 0x3f800000u, 0xbf800001u, 0x00000001u, 0x807fffffu, 0x7f7fffffu,
                          0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc12345u, 0x7f800001u, 0xffbfffffu};  // -0, denormals, inf, quiet and signalling NaNs
  const size_t np = sizeof(pat) / sizeof(pat[0]);
  for (size_t i = 0; i < np; i++) {
    scn_v2f r;
    std::memcpy(&r.x, &pat[i], 4);
    std::memcpy(&r.y, &pat[(i + 5) % np], 4);
    int a = 1, b = 1;
    W::ints(r, a, b);
    CHECK(a == 0 && b == 0);
    const cf c3 = W::conv(r, 7, -9), c4 = W::conv(r, 7, -9, convert_scale(SCN_K_FLOAT_COMPLEX, 12));
    uint32_t g[4];
    std::memcpy(&g[0], &c3.x, 4), std::memcpy(&g[1], &c3.y, 4), std::memcpy(&g[2], &c4.x, 4), std::memcpy(&g[3], &c4.y, 4);
    CHECK(g[0] == pat[i] && g[1] == pat[(i + 5) % np] && g[2] == pat[i] && g[3] == pat[(i + 5) % np]);
  }
}

static void test_bytes() {
  static_assert(scn_wire_bytes(SCN_K_BYTE_COMPLEX) == 2 && scn_wire_bytes(SCN_K_SHORT) == 4 && scn_wire_bytes(SCN_K_SHORT_COMPLEX) == 4 &&
                    scn_wire_bytes(SCN_K_FLOAT_COMPLEX) == 8 && scn_wire_bytes(0) == 0 && scn_wire_bytes(5) == 0,
                "bytes per sample");
  for (uint32_t kind = 0; kind <= 5; kind++) CHECK(bytes_per_sample(kind) == scn_wire_bytes(kind));
  CHECK(SCN_K_BYTE_COMPLEX == SCN_KIND_BYTE_COMPLEX && SCN_K_SHORT == SCN_KIND_SHORT && SCN_K_SHORT_COMPLEX == SCN_KIND_SHORT_COMPLEX &&
        SCN_K_FLOAT_COMPLEX == SCN_KIND_FLOAT_COMPLEX);
}

int main() {
  test_int16();
  test_int8();
  test_float();
  test_bytes();
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("wire tests ok\n");
  return 0;
}
