// scn_average.hip -- averaged (Bartlett) frequency-domain plans: scn_plan_desc.average = K > 1.
//
// A submit of K*G buffers forms G groups of K buffers (SCN_AVG_DWELL: buffers gK .. gK+K-1; SCN_AVG_SWEEPS: g, g+G, ...,
// g+(K-1)G).  Every buffer goes through K1 (convert, with per-buffer DC removal), K2 (window) and K3 (the forward FFT) exactly
// as in scn_fft_kernel; the group's spectrum is P[j] = (sum_b |X_b[j]|^2) / K, then K4 (the dB map) and K5 (mask, threshold,
// records) run once per group.
//
//   scn_avg_power_kernel    persistent workgroups over work items (group g, part q): the transform of scn_fft_kernel
//                           (scn_kernels.hip) on the one geometry both take from scn_device.h (Geo<M>, out_reg<M>: the
//                           n = T a + M b + c decomposition and the LDS layouts); passes 1 - 3 with the prefetch of the next
//                           buffer's samples are written out in both kernels, line for line (as one shared function every
//                           kernel of both families is scheduled differently: profiles/refactor_isa_digest.md), but
//                           the thread's output powers are ADDED into VGPR accumulators.  At the end of an item:
//                           P = 1 (OUT != OUT_PARTIAL): the item is the whole group, and the kernel runs K4 + K5 itself --
//                             db_of_power for the spectrum, the hits-only decision (candidate by linear power p > p_lo, then
//                             db_of_power(p) > threshold inside the mask) for the records, a counter in LDS;
//                           P > 1 (OUT_PARTIAL): the linear partial sum of buffers [q K / P, (q + 1) K / P) goes out.
//   scn_avg_combine_kernel  P > 1 only, per (group, 64 bins): adds the P partial sums in a fixed order (part q in wave q % W,
//                           in part order; then the W wave sums in wave order), divides by K and runs the same K4 + K5.
//                           With P = 1 the two routes would give the same bits; the three output modes agree bit for bit.
//
// 8192 points (H = 2): two 4096-point transforms per buffer, of the even and of the odd samples (the 4096-point kernel's
// passes on a stride-2 view), and the radix-2 step X[k] = E[k] + W_8192^k O[k], X[k + 4096] = E[k] - W_8192^k O[k] in DOUBLE,
// with W in double, each power rounded to float once (the plain 8192-point kernel meets the parity bar with 1.2 % margin; this
// step keeps the averaged one from adding a float butterfly of its own).  A thread then owns 32 bins.
//
// No float atomics anywhere: a result depends on (G, K, P) only, never on timing.  P (scn_avg_parts) comes from the CU
// count, so a group of many buffers -- a single-frequency dwell, G = 1 -- spreads over the whole GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "scn_device.h"
#include "scn_dispatch.h"
#include "scn_kernels.h"

// Build-time split as in scn_kernels.hip: SCN_AVG_TU 0 .. 3 instantiate the kernels of one size (1024, 2048, 4096, 8192);
// TU 3 also holds the combine kernel and the host entry points.  Without SCN_AVG_TU (-1) one translation unit holds everything.
#ifndef SCN_AVG_TU
#define SCN_AVG_TU -1
#endif
#define SCN_AVG_IN_TU(x) (SCN_AVG_TU == -1 || SCN_AVG_TU == (x))

typedef float v32f __attribute__((ext_vector_type(32)));

enum { OUT_PARTIAL = 0, OUT_SPEC = 1, OUT_HITS = 2, OUT_BOTH = 3 };

namespace {

// Geo<M> (scn_device.h) for a buffer of H halves, each one transform of 256 M points
template <int M, int H>
struct AvgGeo : Geo<M> {
  static_assert(H == 1 || (H == 2 && M == 16), "8192 points as two 4096-point halves");
  static constexpr uint32_t NT = Geo<M>::N * H;  // buffer = plan size
  static constexpr uint32_t LDS_BYTES = Geo<M>::EXCH * 8u + Geo<M>::T * 8u + 32u * 4u + 4u;
  static constexpr uint32_t WAVES_PER_SIMD = H == 1 ? 3 : 2;  // H = 2 keeps the even half's 16 outputs and 32 sums besides
  static constexpr uint32_t WG_PER_CU = (WAVES_PER_SIMD * 4u) / Geo<M>::WAVES;
  static constexpr int NB = 16 * H;  // outputs (bins) per thread
};

// The walk of one workgroup over its items w = blockIdx.x + i gridDim.x, inside an item over the part's buffers, inside a
// buffer over its H halves.  Everything here is wave-uniform.
template <int H>
struct AvgCursor {
  uint32_t w, k, k_end, h;  // item, position of the current buffer in its group, end of the part, half
  __device__ __forceinline__ void start_item(const ScnAvgArgs &a) {
    const uint32_t q = w % a.parts;
    k = (uint32_t)(((uint64_t)q * a.k) / a.parts);
    k_end = (uint32_t)(((uint64_t)(q + 1u) * a.k) / a.parts);
    h = 0;
  }
  __device__ __forceinline__ bool valid(const ScnAvgArgs &a) const { return w < a.n_groups * a.parts; }
  __device__ __forceinline__ uint32_t buffer(const ScnAvgArgs &a) const {
    const uint32_t g = w / a.parts;
    return a.layout == SCN_AVG_L_SWEEPS ? g + k * a.n_groups : g * a.k + k;
  }
  // true: the item ended with the unit just done (its sums go out)
  __device__ __forceinline__ bool advance(const ScnAvgArgs &a) {
    if (H == 2 && h == 0) {
      h = 1;
      return false;
    }
    h = 0;
    if (++k < k_end) return false;
    w += gridDim.x;
    if (valid(a)) start_item(a);
    return true;
  }
};

}  // namespace

template <int M, int H, int KIND, bool DC, int OUT>
__global__ __launch_bounds__(16 * M, H == 1 ? 3 : 2) void scn_avg_power_kernel(ScnAvgArgs args) {  // (AvgGeo::WAVES_PER_SIMD)
  typedef AvgGeo<M, H> G;
  constexpr int AUX_LD = SCN_AUX_LD;
  constexpr int AUX_ST = SCN_AUX_ST;
  constexpr uint32_t N = G::N, NT = G::NT, T = G::T, P1 = G::P1, P2 = G::P2;
  constexpr int NB = G::NB;
  constexpr bool HITS = OUT == OUT_HITS || OUT == OUT_BOTH;
  constexpr bool SPEC = OUT == OUT_SPEC || OUT == OUT_BOTH;
  typedef RawLoader<KIND> L;
  typedef typename std::conditional<NB == 16, v16f, v32f>::type VEC;  // the sums
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  v2f *lds = reinterpret_cast<v2f *>(smem_raw);
  v2f *lds_tw2 = lds + G::EXCH;                          // [16][M]
  int *lds_cnt = reinterpret_cast<int *>(lds_tw2 + T);  // [32] DC-sum scratch
  int *lds_hits = lds_cnt + 32;                         // [1] the group's hit counter (P = 1)

  const uint32_t t = threadIdx.x;
  const uint32_t p2 = t / M, c2 = t % M;
  const uint32_t lane = t & 63, wave = t >> 6;

  AvgCursor<H> cur;
  cur.w = blockIdx.x;
  if (!cur.valid(args)) return;  // (the launcher starts no more workgroups than items)
  cur.start_item(args);

  // sample s = H (T a + t) + h of a buffer: a stride-H view for the half h (H = 1: the buffer itself)
  auto rsrc_of = [&](uint32_t buf, bool live) {
    return make_rsrc(reinterpret_cast<const char *>(args.raw) + (size_t)buf * (L::kBytes * NT), live ? L::kBytes * NT : 0u);
  };
  typename L::raw_t raw[16];
  {
    const __amdgpu_buffer_rsrc_t r0 = rsrc_of(cur.buffer(args), true);
#pragma unroll
    for (int a = 0; a < 16; a++) raw[a] = L::template load<AUX_LD>(r0, NT, H * t, H * T * a);
  }

  cf tw1[16];  // W_N^(t p) of the transform (H = 2: the 4096-point table of the plan, tw1_table holds the 8192-point one)
#pragma unroll
  for (int p = 1; p < 16; p++) tw1[p] = from_v2f((H == 1 ? args.tw1_table : args.tw1_half)[(p - 1) * T + t]);
  // window taps with the ENOB scale folded in (onebymax is a power of two); H = 2 reads its half's taps per unit instead (from L2:
  // 32 more persistent VGPRs spilled the hit kernels)
  float win0[16];
#pragma unroll
  for (int a = 0; a < 16; a++) win0[a] = H == 1 ? args.window[T * a + t] * args.scale : 0.0f;
  lds_tw2[t] = args.twiddle[(H * 16 * p2 * c2) & (NT - 1)];  // W_{16M}^(c q) = W_NT^(16 H c q)
  if (t == 0) lds_hits[0] = 0;
  __syncthreads();

  v2f *w1 = lds + t;
  v2f *r1 = lds + p2 * P1 + c2;
  v2f *w2 = lds + c2 * P2 + p2;
  v2f *r3 = lds + t;
  const v2f *tw2 = lds_tw2 + c2;
  const uint32_t st_voff = t * 4u;
  // output o < 16 of the transform is bin t + joff_of(o); with H = 2, output 16 + o is that bin + 4096
  auto joff_of = [](int o) -> uint32_t { return T * ((uint32_t)(o & 15) / M) + 256u * ((uint32_t)(o & 15) % M) + N * (uint32_t)(o >> 4); };
  uint32_t keepmask = 0;
  if (HITS) {
#pragma unroll
    for (int o = 0; o < NB; o++) {
      const uint32_t j = t + joff_of(o);
      keepmask |= scn_bin_evaluated(j, j ^ (NT / 2), NT, args) ? (1u << o) : 0u;
    }
  }

  VEC acc;
#pragma unroll
  for (int o = 0; o < NB; o++) acc[o] = 0.0f;
  cf even[H == 2 ? 16 : 1];  // H = 2: the even half's outputs, until the odd half's are there
  int dc_re = 0, dc_im = 0;

  while (cur.valid(args)) {
    const uint32_t item = cur.w, h = cur.h;
    AvgCursor<H> nx = cur;
    const bool item_done = nx.advance(args);
    const bool more = nx.valid(args);

    if (DC && h == 0) {  // integer mean of the whole buffer with the reference's int32 /= uint32 quirk (utility.cpp:77-78)
      int sr = 0, si = 0;
#pragma unroll
      for (int a = 0; a < 16; a++) {
        int re, im;
        L::ints(raw[a], re, im);
        sr += re;
        si += im;
      }
      if constexpr (H == 2) {  // the odd half's samples as well (read again for its transform: from L2)
        const __amdgpu_buffer_rsrc_t rc = rsrc_of(cur.buffer(args), true);
#pragma unroll 4
        for (int a = 0; a < 16; a++) {  // (four at a time: all sixteen in flight spilled the planar hit kernels)
          int re, im;
          L::ints(L::template load<AUX_LD>(rc, NT, H * t + 1u, H * T * a), re, im);
          sr += re;
          si += im;
        }
      }
      sr = wave_sum(sr);
      si = wave_sum(si);
      if (lane == 0) {
        lds_cnt[wave] = sr;
        lds_cnt[16 + wave] = si;
      }
      __syncthreads();
      sr = si = 0;
#pragma unroll
      for (uint32_t w = 0; w < G::WAVES; w++) {
        sr += lds_cnt[w];
        si += lds_cnt[16 + w];
      }
      dc_re = (int)((uint32_t)sr / NT);
      dc_im = (int)((uint32_t)si / NT);
    }

    cf v[16];
#pragma unroll
    for (int a = 0; a < 16; a++) {
      float wa = win0[a];
      if constexpr (H == 2) wa = args.window[H * (T * a + t) + h] * args.scale;
      v[a] = L::conv(raw[a], dc_re, dc_im, 1.0f) * wa;
    }
    // the next unit's samples, fetched while this one is transformed (zero records past the last: the loads return zeros)
    const __amdgpu_buffer_rsrc_t rn = rsrc_of(more ? nx.buffer(args) : 0u, more);
    const uint32_t nh = more ? nx.h : 0u;
    auto prefetch = [&](int a_lo, int a_hi) {
#pragma unroll
      for (int a = 0; a < 16; a++)
        if (a >= a_lo && a < a_hi) raw[a] = L::template load<AUX_LD>(rn, NT, H * t + nh, H * T * a);
    };
    prefetch(0, 6);

    // ---- pass 1: DFT over a, twiddle W_N^(t p) ----
    fft16(v);
#pragma unroll
    for (int p = 0; p < 16; p++) {
      cf y = v[OUT16(p)];
      if (p) y = cmul(y, tw1[p]);
      w1[p * P1] = to_v2f(y);
    }
    __syncthreads();

    // ---- pass 2: DFT over b, twiddle W_{16M}^(c q) ----
#pragma unroll
    for (int b = 0; b < 16; b++) v[b] = from_v2f(r1[b * M]);
    prefetch(6, 11);
    fft16(v);
#pragma unroll
    for (int q = 1; q < 16; q++) v[OUT16(q)] = cmul(v[OUT16(q)], from_v2f(tw2[q * M]));
    __syncthreads();
    prefetch(11, 16);
#pragma unroll
    for (int q = 0; q < 16; q++) w2[q * 16] = to_v2f(v[OUT16(q)]);
    __syncthreads();

    // ---- pass 3: M-point DFT over c ----
#pragma unroll
    for (int u = 0; u < 16 / M; u++)
#pragma unroll
      for (int c = 0; c < M; c++) v[u * M + c] = from_v2f(r3[c * P2 + T * u]);
    if constexpr (M == 16) fft16(v);
    if constexpr (M == 8) {
      fft8(v);
      fft8(v + 8);
    }
    if constexpr (M == 4) {
#pragma unroll
      for (int u = 0; u < 4; u++) radix4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
    }
    // the same thread owns the same bins for every buffer: the group's sums stay in registers
    if constexpr (H == 1) {
#pragma unroll
      for (int o = 0; o < 16; o++) acc[o] = acc[o] + power_of(v[out_reg<M>(o)]);
    } else if (h == 0) {
#pragma unroll
      for (int o = 0; o < 16; o++) even[o] = v[out_reg<M>(o)];
    } else {
#pragma unroll
      for (int o = 0; o < 16; o++) {
        const cf e = even[o], od = v[out_reg<M>(o)];
        const double2_scn w = args.tw_half[t + joff_of(o)];  // W_8192^k, k < 4096, in double
        const double wr = (double)od.x * w.x - (double)od.y * w.y, wi = (double)od.x * w.y + (double)od.y * w.x;
        const double ar = (double)e.x + wr, ai = (double)e.y + wi, br = (double)e.x - wr, bi = (double)e.y - wi;
        acc[o] = acc[o] + (float)(ar * ar + ai * ai);
        acc[16 + o] = acc[16 + o] + (float)(br * br + bi * bi);
      }
    }
    __syncthreads();  // exchange area free again

    if (item_done) {
      if constexpr (OUT == OUT_PARTIAL) {
        const __amdgpu_buffer_rsrc_t rout = make_rsrc(args.partial + (size_t)item * NT, 4u * NT);
#pragma unroll
        for (int o = 0; o < NB; o++) {
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, (float)acc[o]), rout, st_voff, 4u * joff_of(o), AUX_ST);
          acc[o] = 0.0f;
        }
      } else {  // P = 1: item = group; K4 + K5 here, as scn_avg_combine_kernel runs them
        const uint32_t g = item;
        const float kf = (float)args.k;
        // 16 outputs at a time (H = 2: the bins k, then the bins k + 4096 -- one 32-output record pass spilled)
#pragma unroll
        for (int hh = 0; hh < H; hh++) {
          v16f pw;
          float gmax[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int o = 0; o < 16; o++) {
            const float q = acc[16 * hh + o] / kf;  // a true division, as the definition states
            pw[o] = q;
            gmax[o / 4] = fmaxf(gmax[o / 4], q);
            acc[16 * hh + o] = 0.0f;
          }
          if constexpr (SPEC) {
            const __amdgpu_buffer_rsrc_t rout = make_rsrc(args.power_db + (size_t)g * NT, 4u * NT);
#pragma unroll
            for (int o = 0; o < 16; o++)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, db_of_power((float)pw[o])), rout, st_voff, 4u * joff_of(16 * hh + o), AUX_ST);
          }
          if constexpr (HITS) {
            const float pmax = fmaxf(fmaxf(gmax[0], gmax[1]), fmaxf(gmax[2], gmax[3]));
            if (__ballot(pmax > args.p_lo))
              scn_record_hits_lanes<16, false, true>(pw, gmax, (keepmask >> (16 * hh)) & 0xffffu, args, lds_hits, g, lane,
                                                     [&](int o) -> uint32_t { return (t + joff_of(16 * hh + o)) ^ (NT / 2); });
          }
        }
        if constexpr (HITS) {
          __syncthreads();  // every recorder of this group done (the counter is next touched K units of barriers later)
          if (t == 0) {
            args.per_group_hits[g] = (uint32_t)lds_hits[0];
            lds_hits[0] = 0;
          }
        }
      }
    }
    cur = nx;
  }
}

#if SCN_AVG_IN_TU(3)
// One workgroup per (group, 64 consecutive bins), W = blockDim.x / 64 waves: wave x adds parts x, x + W, ... in order; wave 0
// adds the W sums in wave order, divides by K and runs K4 + K5 for its 64 bins (one per lane).
template <bool HITS, bool SPEC>
__global__ __launch_bounds__(1024) void scn_avg_combine_kernel(ScnAvgArgs args) {
  __shared__ float part_sum[16][64];
  const uint32_t N = args.n;
  const uint32_t chunks = N / 64u;
  const uint32_t g = blockIdx.x / chunks;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nw = blockDim.x >> 6;
  const uint32_t j = (blockIdx.x % chunks) * 64u + lane;
  const float *src = args.partial + (size_t)g * args.parts * N + j;
  float s = 0.0f;
  uint32_t q = wave;
  for (; q + 3u * nw < args.parts; q += 4u * nw) {  // four loads in flight per lane, added in part order
    const float a0 = __builtin_nontemporal_load(src + (size_t)q * N);
    const float a1 = __builtin_nontemporal_load(src + (size_t)(q + nw) * N);
    const float a2 = __builtin_nontemporal_load(src + (size_t)(q + 2u * nw) * N);
    const float a3 = __builtin_nontemporal_load(src + (size_t)(q + 3u * nw) * N);
    s = s + a0;
    s = s + a1;
    s = s + a2;
    s = s + a3;
  }
  for (; q < args.parts; q += nw) s = s + __builtin_nontemporal_load(src + (size_t)q * N);
  if (nw > 1u) {
    part_sum[wave][lane] = s;
    __syncthreads();
    if (wave) return;
    s = part_sum[0][lane];
    for (uint32_t x = 1; x < nw; x++) s = s + part_sum[x][lane];
  }
  const float p = s / (float)args.k;  // the mean power of the group (a true division, as the definition states)
  if constexpr (SPEC) {
    const float d = db_of_power(p);
    __builtin_nontemporal_store(d, args.power_db + (size_t)g * N + j);
  }
  if constexpr (HITS) {
    const uint32_t i = j ^ (N / 2u);  // (j + N/2) % N, process.cpp:47
    const bool keep = scn_bin_evaluated(j, i, N, args);
    const bool cand = keep && p > args.p_lo;
    if (!__ballot(cand)) return;
    const float d = db_of_power(p);
    const bool hit = cand && d > args.threshold;  // strict >, process.cpp:54
    const unsigned long long m = __ballot(hit);
    if (!m) return;
    uint32_t base = 0;
    if (lane == 0) base = (uint32_t)atomicAdd(args.per_group_hits + g, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (hit) {
      const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (pos < args.hit_region) args.hits[(size_t)g * args.hit_region + pos] = ScnDevHit{i, d};
    }
  }
}
#endif

// a launch of the power kernel on its way to the translation unit that holds the size's kernels
struct ScnAvgLaunch {
  int kind;
  bool dc, split, hits, spec;  // split: partial sums go out (parts > 1); else the output mode
  const ScnAvgArgs &a;
  uint32_t grid;
  hipStream_t s;
};

namespace {
// resident workgroups per CU of the power kernel: 12 / 6 / 3 / 2 at 1024 / 2048 / 4096 / 8192 points
uint32_t avg_wg_per_cu(uint32_t n) {
  return n == 1024 ? AvgGeo<4, 1>::WG_PER_CU : n == 2048 ? AvgGeo<8, 1>::WG_PER_CU : n == 4096 ? AvgGeo<16, 1>::WG_PER_CU : AvgGeo<16, 2>::WG_PER_CU;
}

template <int M, int H>
hipError_t launch_power(const ScnAvgLaunch &l) {
  typedef AvgGeo<M, H> G;
  return scn_with_kind(l.kind, l.dc, [&](auto kind, auto dc) {
    auto launch = [&](auto out) {
      hipLaunchKernelGGL((scn_avg_power_kernel<M, H, decltype(kind)::value, decltype(dc)::value, decltype(out)::value>), dim3(l.grid), dim3(G::T),
                         G::LDS_BYTES, l.s, l.a);
      return hipGetLastError();
    };
    if (l.split) return launch(std::integral_constant<int, OUT_PARTIAL>{});
    return scn_with_mode(l.hits, l.spec, [&](auto hits, auto spec) {
      return launch(std::integral_constant<int, (decltype(hits)::value ? OUT_HITS : 0) | (decltype(spec)::value ? OUT_SPEC : 0)>{});
    });
  });
}
}  // namespace

// one launcher per translation unit, as scn_launch_fft_unit (scn_kernels.hip): unit u holds M = 4, 8, 16 and 16 with H = 2
template <int TU>
hipError_t scn_launch_avg_unit(const ScnAvgLaunch &l);
#if SCN_AVG_TU == -1
template <int TU>
hipError_t scn_launch_avg_unit(const ScnAvgLaunch &l) { return launch_power<(TU < 3 ? 4 << TU : 16), (TU < 3 ? 1 : 2)>(l); }
#else
template <>
hipError_t scn_launch_avg_unit<SCN_AVG_TU>(const ScnAvgLaunch &l) { return launch_power<(SCN_AVG_TU < 3 ? 4 << SCN_AVG_TU : 16), (SCN_AVG_TU < 3 ? 1 : 2)>(l); }
#endif

#if SCN_AVG_IN_TU(3)
uint32_t scn_avg_parts(uint32_t n, uint32_t n_groups, uint32_t k, int num_cus) {
  if (!n_groups || k <= 1u) return 1u;
  const uint32_t slots = (uint32_t)num_cus * avg_wg_per_cu(n);
  if (n_groups >= slots) return 1u;
  const uint32_t want = (slots + n_groups - 1u) / n_groups;  // enough items to give every workgroup slot one
  const uint32_t cap = (k + 1u) / 2u;                         // at least two buffers per part (the last one may hold one)
  return want < cap ? want : cap;
}

size_t scn_avg_partial_floats(uint32_t n, uint32_t max_groups, int num_cus) {
  // partial sums exist only when P > 1, i.e. G < slots, and then G P < slots + G <= 2 slots
  return 2u * (size_t)num_cus * avg_wg_per_cu(n) * n;
}

hipError_t scn_launch_average(int kind, bool correct_dc, bool hits, bool spectrum, const ScnAvgArgs &a, int num_cus, hipStream_t s) {
  if (!a.n_groups) return hipSuccess;
  const bool split = a.parts > 1u;
  // items spread evenly: ceil(items / slots) items per workgroup, and the fewest workgroups that cover them at that rate (the
  // last ones may take one item fewer; at G = 1024, P = 1, 4096 points: 512 workgroups of two items, a third of the slots idle)
  const uint32_t items = a.n_groups * a.parts, slots = (uint32_t)num_cus * avg_wg_per_cu(a.n);
  const uint32_t per = (items + slots - 1u) / slots;
  const uint32_t grid = (items + per - 1u) / per;
  if (!scn_avg_size_supported(a.n)) return hipErrorInvalidValue;
  static constexpr hipError_t (*units[4])(const ScnAvgLaunch &) = {scn_launch_avg_unit<0>, scn_launch_avg_unit<1>, scn_launch_avg_unit<2>, scn_launch_avg_unit<3>};
  hipError_t e = units[__builtin_ctz(a.n) - 10](ScnAvgLaunch{kind, correct_dc, split, hits, spectrum, a, grid, s});
  if (e != hipSuccess || !split) return e;
  if (hits && (e = hipMemsetAsync(a.per_group_hits, 0, sizeof(uint32_t) * a.n_groups, s)) != hipSuccess) return e;
  const uint32_t waves = a.parts < 16u ? a.parts : 16u;
  const dim3 cgrid(a.n_groups * (a.n / 64u)), block(64u * waves);
  return scn_with_mode(hits, spectrum, [&](auto h, auto sp) {
    hipLaunchKernelGGL((scn_avg_combine_kernel<decltype(h)::value, decltype(sp)::value>), cgrid, block, 0, s, a);
    return hipGetLastError();
  });
}
#endif
