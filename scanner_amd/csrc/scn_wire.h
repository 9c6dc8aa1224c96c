// scn_wire.h -- K1, the four wire formats, stated once: bytes per sample, the register form of a sample and its decode
// (utility.cpp:9-84).  Every kernel family fetches samples its own way (RawLoader, BigRaw, WelchRaw, the plain pointer of
// scn_generic.hip) and decodes them here.  No HIP header: tests/cpp/test_wire.cpp builds this with g++ and holds every
// value of it against the oracle's conversions.
#pragma once
#include <stdint.h>

#include "scn_mask.h"  // SCN_HOST_DEVICE

// same numbering as messageQueue.h:31-37 / SCN_KIND_*
#define SCN_K_BYTE_COMPLEX 1
#define SCN_K_SHORT 2
#define SCN_K_SHORT_COMPLEX 3
#define SCN_K_FLOAT_COMPLEX 4

#ifdef __clang__
typedef float scn_v2f __attribute__((ext_vector_type(2)));  // memory / LDS element (8 B)
#else
struct scn_v2f {
  float x, y;
};
#endif

// Register-resident complex value.  Deliberately two independent floats, not an
// ext_vector: on gfx950 a v_pk_*_f32 costs the same 4 issue cycles as two scalar ops, and
// hipcc's packed complex multiply is 3 packed ops + a move + wait states (~14 cycles)
// against 8 for mul/mul/fma/fma, so scalar arithmetic is the faster form here.
struct cf {
  float x, y;
};

// Wire<KIND>: kBytes per sample; raw_t, a sample in a register; ints(), its two integers (the DC sums; float samples have
// none: no DC removal, messageQueue.h:229-236); conv(raw, dc_re, dc_im) = float(source - dc), utility.cpp:81-82, in wrapping
// uint32 arithmetic like the oracle's conv1; conv(..., scale) = that times onebymax.  Where the scale rides in the window
// taps instead (the four-step kernels) the product rounds identically: onebymax is +-2^-k.
template <int KIND>
struct Wire;

// what the integer formats share: W supplies ints()
template <class W>
struct WireInt {
  typedef int raw_t;
  static SCN_HOST_DEVICE cf conv(raw_t r, int dc_re, int dc_im) {
    int re, im;
    W::ints(r, re, im);
    return cf{(float)(int)((uint32_t)re - (uint32_t)dc_re), (float)(int)((uint32_t)im - (uint32_t)dc_im)};
  }
  // (written out, not conv(r, dc_re, dc_im) times scale: through that call scn_time_domain_wave_kernel<SCN_K_SHORT, true> came out in
  //  another instruction order, profiles/wire_once.md)
  static SCN_HOST_DEVICE cf conv(raw_t r, int dc_re, int dc_im, float scale) {
    int re, im;
    W::ints(r, re, im);
    return cf{(float)(int)((uint32_t)re - (uint32_t)dc_re) * scale, (float)(int)((uint32_t)im - (uint32_t)dc_im) * scale};
  }
};

// float I,Q interleaved: a copy (the plan's scale is 1 and is not applied: a NaN keeps its payload)
template <>
struct Wire<SCN_K_FLOAT_COMPLEX> {
  static constexpr uint32_t kBytes = 8;
  typedef scn_v2f raw_t;
  static SCN_HOST_DEVICE void ints(raw_t, int &re, int &im) { re = im = 0; }
  static SCN_HOST_DEVICE cf conv(raw_t r, int, int) { return cf{r.x, r.y}; }
  static SCN_HOST_DEVICE cf conv(raw_t r, int, int, float) { return cf{r.x, r.y}; }
};

// int16 I,Q interleaved: re | im << 16
template <>
struct Wire<SCN_K_SHORT_COMPLEX> : WireInt<Wire<SCN_K_SHORT_COMPLEX>> {
  static constexpr uint32_t kBytes = 4;
  static SCN_HOST_DEVICE void ints(raw_t r, int &re, int &im) {
    re = (int)(short)(r & 0xffff);
    im = r >> 16;
  }
};

// int16 planar, I[n] then Q[n] per buffer: the loaders pack a sample into the interleaved register form
template <>
struct Wire<SCN_K_SHORT> : Wire<SCN_K_SHORT_COMPLEX> {};

// int8 I,Q interleaved: bytes 0 and 1 of the register (the rest is never read)
template <>
struct Wire<SCN_K_BYTE_COMPLEX> : WireInt<Wire<SCN_K_BYTE_COMPLEX>> {
  static constexpr uint32_t kBytes = 2;
  static SCN_HOST_DEVICE void ints(raw_t r, int &re, int &im) {
    re = (int)(signed char)(r & 0xff);
    im = (int)(signed char)((r >> 8) & 0xff);
  }
};

// bytes per sample of a wire format; 0: unknown kind
constexpr uint32_t scn_wire_bytes(uint32_t kind) {
  return kind == SCN_K_BYTE_COMPLEX    ? Wire<SCN_K_BYTE_COMPLEX>::kBytes
         : kind == SCN_K_SHORT         ? Wire<SCN_K_SHORT>::kBytes
         : kind == SCN_K_SHORT_COMPLEX ? Wire<SCN_K_SHORT_COMPLEX>::kBytes
         : kind == SCN_K_FLOAT_COMPLEX ? Wire<SCN_K_FLOAT_COMPLEX>::kBytes
                                       : 0u;
}
