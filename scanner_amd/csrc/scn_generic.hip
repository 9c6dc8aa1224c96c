// scn_generic.hip -- the same per-buffer path for the FFT sizes no fused kernel covers: Bluestein's algorithm.
//
// The reference plans an FFT for whatever --count it is given (fft.cpp:4-11, scan.cpp:85).  Every power of two from 16 to
// 65536 has a fused or four-step kernel, and so have the 5-smooth sizes of scn_mixed_plans.h; every other size from 16 to
// 65535 runs here, through HBM, around Bluestein's identity
//   X[k] = w[k] * sum_n (x[n] w[n]) conj(w)[k - n],   w[n] = exp(-i pi n^2 / N):
// a cyclic convolution of length M = the power of two >= 2N - 1, transformed stage by stage:
//
//   scn_gen_load_kernel       K1 + K2: raw wire format -> complex float, DC removal, window (utility.cpp:9-84, process.cpp:28-34),
//                             times w, zero-padded to M
//   scn_gen_stage_kernel      one out-of-place Stockham stage of radix 16, 4 or 2: after log_R M launches the transform is in
//                             natural order
//   scn_gen_pointwise_kernel  times the precomputed FFT_M of the chirp filter (scaled by 1/M), conjugated; then the stages
//                             again (an inverse transform up to a conjugation)
//   scn_gen_finish_kernel     K4 + K5: dB (utility.cpp:86-98), fftshift-indexed mask, strict > threshold, hit records into the
//                             buffer's region (process.cpp:46-62)
//
// The final w[k] and the conjugation have modulus one and never reach the dB value.  The same outputs as the fused path
// (spectrum, per-buffer counts, unordered regions that scn_hits.hip orders), in double between input and spectrum: a
// correctness path for unusual sizes, not a fast one -- each kernel is a plain streaming kernel (coalesced reads; the stage
// writes are strided by the sub-transform length).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "scn_device.h"
#include "scn_dispatch.h"
#include "scn_kernels.h"

namespace {

// Everything between the windowed input and the final spectrum is DOUBLE: the work buffers, the twiddle / chirp / filter
// tables and the butterflies; the spectrum is rounded to float once, in the finish kernel -- the accuracy class of the
// oracle's default mode (and of FFTW's float transform, which it stands in for).  The first version kept float work
// buffers: eight stages then round a strong tone's partial sums to float eight times (the fused kernels: three), and a
// buffer with peak/mean power 8e3 at 32768 points read 1.0e-5 .. 1.2e-5 on bins near the mean -- AT the parity bar.  This
// is the correctness path for unusual sizes; it is bound by its HBM passes, and it pays for the wider ones.
// sample i of an n-sample buffer in Wire<KIND>'s register form, from the plain pointer
template <int KIND>
__device__ __forceinline__ typename Wire<KIND>::raw_t gen_fetch(const void *buf, uint32_t n, uint32_t i) {
  if constexpr (KIND == SCN_K_FLOAT_COMPLEX) return static_cast<const v2f *>(buf)[i];
  else if constexpr (KIND == SCN_K_SHORT_COMPLEX) return static_cast<const int *>(buf)[i];
  else if constexpr (KIND == SCN_K_BYTE_COMPLEX)  // (two byte loads: the load kernel's code as it was, profiles/wire_once.md)
    return (int)static_cast<const unsigned char *>(buf)[2 * i] | ((int)static_cast<const unsigned char *>(buf)[2 * i + 1] << 8);
  else return (int)static_cast<const unsigned short *>(buf)[i] | ((int)static_cast<const unsigned short *>(buf)[n + i] << 16);  // planar: I[n] then Q[n]
}

template <int KIND, bool DC>
__global__ __launch_bounds__(256) void scn_gen_load_kernel(ScnGenericArgs a) {
  typedef Wire<KIND> L;
  __shared__ int s_sum[8];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t n = a.n;
  for (uint32_t b = blockIdx.x; b < a.n_buffers; b += gridDim.x) {
    const char *buf = static_cast<const char *>(a.raw) + (size_t)b * L::kBytes * n;
    int dc_re = 0, dc_im = 0;
    if (DC) {
      int sr = 0, si = 0;
      for (uint32_t i = t; i < n; i += 256u) {
        int re, im;
        L::ints(gen_fetch<KIND>(buf, n, i), re, im);
        sr += re;
        si += im;
      }
      sr = wave_sum(sr);
      si = wave_sum(si);
      __syncthreads();  // s_sum free again
      if (lane == 0) {
        s_sum[wave] = sr;
        s_sum[4 + wave] = si;
      }
      __syncthreads();
      dc_re = (int)((uint32_t)(s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]) / n);  // int32 /= uint32, utility.cpp:77-78
      dc_im = (int)((uint32_t)(s_sum[4] + s_sum[5] + s_sum[6] + s_sum[7]) / n);
    }
    scn_v2d *out = static_cast<scn_v2d *>(a.work0) + (size_t)b * a.m;
    // the windowed sample is a FLOAT product, as in the reference (process.cpp:28-34 multiplies floats) and in the fused
    // kernels: float(s - dc)*onebymax*w and float(s - dc)*(onebymax*w) round identically (onebymax is +-2^-k)
    // times the chirp, zero-padded to the convolution length
    for (uint32_t i = t; i < a.m; i += 256u) {
      cd v = cd{0.0, 0.0};
      if (i < n) {
        const cf x = L::conv(gen_fetch<KIND>(buf, n, i), dc_re, dc_im) * (a.window[i] * a.scale);
        // (the written-out FMA form: left to the compiler, the contraction of x w = (x.x w.x - x.y w.y, ...) came out differently
        //  in the int16 instantiation than in the others, and a constant buffer's residue bins differed between wire formats)
        const scn_v2d c = static_cast<const scn_v2d *>(a.chirp)[i];
        v = cmul_d(cd{(double)x.x, (double)x.y}, c.x, c.y);
      }
      out[i] = to_v2d(v);
    }
  }
}

// Bluestein, between the two transforms: y = conj(x * B'), B' = FFT_M(chirp filter) / M
__global__ __launch_bounds__(256) void scn_gen_pointwise_kernel(ScnGenericArgs a, scn_v2d *__restrict__ x) {
  const size_t total = (size_t)a.n_buffers << a.log2m;
  for (size_t g = (size_t)blockIdx.x * 256u + threadIdx.x; g < total; g += (size_t)gridDim.x * 256u) {
    const cd y = cmul_d(from_v2d(x[g]), static_cast<const scn_v2d *>(a.bfilter)[(uint32_t)g & (a.m - 1u)]);
    x[g] = scn_v2d{y.x, -y.y};
  }
}

// One Stockham stage of radix R over every buffer of the batch.  Butterfly j in [0, N/R) of a stage whose finished
// sub-transforms have length Ns reads x[j + r N/R], multiplies by W_{R Ns}^{r (j mod Ns)} = W_N^{r (j mod Ns) N/(R Ns)},
// does the R-point DFT and writes y[(j / Ns) R Ns + (j mod Ns) + r Ns].  Ns = 1, R, R^2, ... : natural order in, natural
// order out after the last stage.
template <int R>
__global__ __launch_bounds__(256) void scn_gen_stage_kernel(ScnGenericArgs a, const scn_v2d *__restrict__ src, scn_v2d *__restrict__ dst,
                                                            uint32_t log2ns) {
  // every quantity is a power of two: shifts and masks, no integer division (the first version divided: 10 ms per
  // 512 x 65536-point batch instead of ~2)
  constexpr uint32_t LR = R == 16 ? 4u : R == 4 ? 2u : 1u;
  const uint32_t n = a.m, log2n = a.log2m, log2per = log2n - LR, per = 1u << log2per, ns = 1u << log2ns;  // the transform length
  const size_t total = (size_t)a.n_buffers << log2per;
  for (size_t g = (size_t)blockIdx.x * 256u + threadIdx.x; g < total; g += (size_t)gridDim.x * 256u) {
    const uint32_t b = (uint32_t)(g >> log2per), j = (uint32_t)g & (per - 1u);
    const scn_v2d *x = src + ((size_t)b << log2n);
    scn_v2d *y = dst + ((size_t)b << log2n);
    const uint32_t k = j & (ns - 1u);
    const uint32_t step = n >> (LR + log2ns);  // twiddle index stride in the W_N table
    const uint32_t j0 = ((j >> log2ns) << (log2ns + LR)) + k;
    if constexpr (R == 16) {
      cd v[16];
#pragma unroll
      for (int r = 0; r < 16; r++) v[r] = from_v2d(x[j + r * per]);
      if (k) {
        const scn_v2d *tw = static_cast<const scn_v2d *>(a.twiddle);
#pragma unroll
        for (int r = 1; r < 16; r++) v[r] = cmul_d(v[r], tw[r * k * step]);   // r k step < n: no wrap
      }
      fft16_d(v);
#pragma unroll
      for (int r = 0; r < 16; r++) y[j0 + r * ns] = to_v2d(v[4 * (r & 3) + (r >> 2)]);
    } else if constexpr (R == 4) {
      cd v0 = from_v2d(x[j]), v1 = from_v2d(x[j + per]), v2 = from_v2d(x[j + 2 * per]), v3 = from_v2d(x[j + 3 * per]);
      if (k) {
        const scn_v2d *tw = static_cast<const scn_v2d *>(a.twiddle);
        v1 = cmul_d(v1, tw[k * step]);
        v2 = cmul_d(v2, tw[2 * k * step]);
        v3 = cmul_d(v3, tw[3 * k * step]);
      }
      radix4_d(v0, v1, v2, v3);
      y[j0] = to_v2d(v0);
      y[j0 + ns] = to_v2d(v1);
      y[j0 + 2 * ns] = to_v2d(v2);
      y[j0 + 3 * ns] = to_v2d(v3);
    } else {
      cd v0 = from_v2d(x[j]), v1 = from_v2d(x[j + per]);
      if (k) v1 = cmul_d(v1, static_cast<const scn_v2d *>(a.twiddle)[k * step]);
      y[j0] = to_v2d(v0 + v1);
      y[j0 + ns] = to_v2d(v0 - v1);
    }
  }
}

template <bool HITS>
__global__ __launch_bounds__(256) void scn_gen_finish_kernel(ScnGenericArgs a, const scn_v2d *__restrict__ spec) {
  const uint32_t n = a.n;
  const size_t total = (size_t)a.n_buffers * n;
  for (size_t g = (size_t)blockIdx.x * 256u + threadIdx.x; g < total; g += (size_t)gridDim.x * 256u) {
    const uint32_t b = (uint32_t)(g / n), j = (uint32_t)(g - (size_t)b * n);
    const scn_v2d X = spec[((size_t)b << a.log2m) + j];  // rows are m long
    const float d = power_db(cf{(float)X.x, (float)X.y});  // the spectrum in float (fft.cpp:20-25 delivers floats), then utility.cpp:86-98
    if (a.power_db) a.power_db[g] = d;
    if (HITS) {
      const uint32_t i = (j + n - n / 2u) % n;  // the i with (i + N/2) % N == j, process.cpp:47
      const bool keep = scn_bin_evaluated(j, i, n, a);
      const bool hit = keep && d > a.threshold;  // strict >, process.cpp:54
      if (hit) {
        const uint32_t pos = atomicAdd(&a.per_buffer_hits[b], 1u);
        if (pos < a.hit_region) a.hits[(size_t)b * a.hit_region + pos] = ScnDevHit{i, d};
      }
    }
  }
}

}  // namespace

hipError_t scn_launch_generic(int kind, bool dc, bool hits, const ScnGenericArgs &a, int num_cus, hipStream_t s) {
  if (a.n_buffers == 0) return hipSuccess;
  hipError_t e = hipSuccess;
  if (hits) {
    e = hipMemsetAsync(a.per_buffer_hits, 0, sizeof(uint32_t) * a.n_buffers, s);
    if (e != hipSuccess) return e;
  }
  const int resident = num_cus * 8;
  const int load_grid = (int)((uint32_t)resident < a.n_buffers ? (uint32_t)resident : a.n_buffers);
  e = scn_with_kind(kind, dc, [&](auto k, auto d) {
    hipLaunchKernelGGL((scn_gen_load_kernel<decltype(k)::value, decltype(d)::value>), dim3(load_grid), dim3(256), 0, s, a);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  auto blocks_for = [&](size_t items) {
    size_t b = (items + 255u) / 256u;
    const size_t cap = (size_t)resident * 4u;
    return (int)(b < cap ? b : cap);
  };
  // forward transform of length m from `from`, ping-ponging with the other work buffer; returns where the result is:
  // log2 m = 4 s + r: one radix-2 stage if r is odd, one radix-4 stage if r >= 2, radix 16 from there on -- every stage is a
  // pass over the batch in double (32 B per point), so the fewer the better: 65536 points in 4 passes, 512 in 3
  auto transform = [&](scn_v2d *from, scn_v2d *other) -> scn_v2d * {
    scn_v2d *src = from, *dst = other;
    uint32_t log2ns = 0;
    if (a.log2m & 1u) {
      hipLaunchKernelGGL((scn_gen_stage_kernel<2>), dim3(blocks_for((size_t)a.m / 2 * a.n_buffers)), dim3(256), 0, s, a, src, dst, log2ns);
      log2ns += 1;
      std::swap(src, dst);
    }
    if (a.log2m & 2u) {
      hipLaunchKernelGGL((scn_gen_stage_kernel<4>), dim3(blocks_for((size_t)a.m / 4 * a.n_buffers)), dim3(256), 0, s, a, src, dst, log2ns);
      log2ns += 2;
      std::swap(src, dst);
    }
    while (log2ns < a.log2m) {
      hipLaunchKernelGGL((scn_gen_stage_kernel<16>), dim3(blocks_for((size_t)a.m / 16 * a.n_buffers)), dim3(256), 0, s, a, src, dst, log2ns);
      log2ns += 4;
      std::swap(src, dst);
    }
    return src;
  };
  scn_v2d *const w0 = static_cast<scn_v2d *>(a.work0), *const w1 = static_cast<scn_v2d *>(a.work1);
  scn_v2d *spec = transform(w0, w1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // multiply by the filter's transform, conjugate, transform again
  hipLaunchKernelGGL(scn_gen_pointwise_kernel, dim3(blocks_for((size_t)a.m * a.n_buffers)), dim3(256), 0, s, a, spec);
  spec = transform(spec, spec == w0 ? w1 : w0);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int fin = blocks_for((size_t)a.n * a.n_buffers);
  if (hits) hipLaunchKernelGGL((scn_gen_finish_kernel<true>), dim3(fin), dim3(256), 0, s, a, spec);
  else hipLaunchKernelGGL((scn_gen_finish_kernel<false>), dim3(fin), dim3(256), 0, s, a, spec);
  return hipGetLastError();
}
