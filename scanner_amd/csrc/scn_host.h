// scn_host.h -- the C-ABI layer's arithmetic that never touches HIP (scn_host.hip).  Plain C++: tests/cpp/test_plan_math.cpp
// compiles the unit with g++ and no HIP header on the include path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/scanner_hip.h"
#include "scn_mask.h"

// The layer's one error setter: formats the text scn_last_error returns (one thread_local for the whole library), returns `status`
int scn_fail(int status, const char *fmt, ...);

size_t bytes_per_sample(uint32_t kind);  // 0: unknown kind
float convert_scale(uint32_t kind, uint32_t enob);
bool build_window(uint32_t type, uint32_t n, std::vector<float> &w);  // false: unknown type
void host_fft(std::vector<double> &re, std::vector<double> &im);
// W_m^k = exp(-2 pi i k / m), k < m, as (re, im) pairs, evaluated in double (T: float or double)
template <class T>
std::vector<T> twiddles(uint32_t m);

// What a Bluestein plan of n points reads, in double: m = 2^log2m >= 2n - 1; twiddle [m][2], chirp [n][2], bfilter [m][2]
struct ScnBluesteinTables {
  uint32_t m = 0, log2m = 0;
  std::vector<double> twiddle, chirp, bfilter;
};
ScnBluesteinTables bluestein_tables(uint32_t n);

bool floor_permille_of(uint32_t given, uint32_t *permille);
uint32_t evaluated_bins(uint32_t n, uint32_t dc_ignore, double use_bandwidth, uint32_t *i_lo, uint32_t *i_hi);
// The floor window (scanner_hip.h, "Floor window") on a mask with the defaults applied: need[i] = r_i + 1 -- the number of reference
// cells that must lie below bin i for it to be a hit -- for every evaluated fftshift index i, 0 for the others.  SCN_E_INVALID (with
// the error text set, `need` unspecified) for a window outside the limits or one that leaves an evaluated bin without a cell.
int floor_window_ranks(uint32_t n, uint32_t dc_ignore, uint32_t i_lo, uint32_t i_hi, uint32_t permille, uint32_t train, uint32_t guard,
                       std::vector<uint16_t> &need);

// Baseline plans (scanner_hip.h, "Baseline detector"): what a submit, an update and a read-out must satisfy, from numbers alone
// (SCN_OK, or the status with the error text set).  rows: the baseline's; indexed: the submit names a run of the plan's table
int check_baseline_submit(uint32_t rows, bool indexed, uint32_t table_count);
int check_baseline_update(uint32_t rows, uint32_t units, uint32_t op);
int check_baseline_range(uint32_t have, uint32_t first_row, uint32_t rows);

// Averaged plans (k = average > 1; sweeps: SCN_AVG_SWEEPS, else SCN_AVG_DWELL).  group_headers redirects fc / seq to the groups'
// (held in group_fc / group_seq) where the submit gave them or the compaction kernel's default would be wrong; returns the groups
int check_average(uint32_t k, bool sweeps, uint32_t nb, const double *fc);
uint32_t group_headers(uint32_t k, bool sweeps, uint32_t nb, const double *&fc, const uint64_t *&seq, std::vector<double> &group_fc,
                       std::vector<uint64_t> &group_seq);

// The route of a submit: what follows the transform, on which stream, behind which event -- decided once by submit_route from the
// numbers below and only executed by submit_common (scn_submit.hip); tests/cpp/test_submit_route.cpp enumerates the table.
// The thresholds (each measured: the notes stand at the branches of submit_route, scn_host.hip):
#ifndef SCN_TOTAL_KERNEL_FROM
#define SCN_TOTAL_KERNEL_FROM (1u << 18)
#endif
constexpr uint32_t kTotalKernelFrom = SCN_TOTAL_KERNEL_FROM;  // units per launch from which a reduction on the GPU replaces the counts' DMA
constexpr uint32_t kStoredCountsUpTo = 4096;                  // units per launch up to which a fused kernel stores the counts to pinned memory itself
constexpr uint64_t kPacketEventFrom = 1ull << 25;             // samples per launch from which a fused kernel's own dispatch packet completes the event

struct SubmitShape {
  bool hits;           // the plan reports hits (SCN_OUT_HITS)
  bool fused;          // the transform is the submit's last kernel and can store counts and complete an event itself: a fused path, not averaged, no detect kernel behind it
  bool direct_counts;  // the plan's (scn_plan::direct_counts; fused plans only)
  bool own_stream;     // the slot has a stream of its own (SCN_PLAN_OVERLAP_SLOTS)
  bool list_wanted;    // the plan's previous collect took records or a device list
  uint32_t n, units;   // points per transform; buffers per launch, or groups on an averaged plan
};
enum class Counts { None, Stored, Dma, Reduced };  // no hits or no units; by the kernel's own stores to pinned memory; by a DMA; the total + trigger bitmap of scn_hit_total_kernel
enum class RouteStream { Slot, D2H };
enum class KernelEnd { None, Done, KernelDone };  // the event that marks the end of the submit's last compute kernel
struct SubmitRoute {
  Counts counts = Counts::None;
  RouteStream counts_stream = RouteStream::Slot;  // carries the counts, a floor plan's floors and `done` behind them; D2H waits for `end`
  bool list_behind = false;                       // the ordered list is built behind the launch ...
  bool list_forks = false;                        // ... on the plan's list stream, which waits for `end` (else: on the slot's own)
  KernelEnd end = KernelEnd::None;
  bool end_in_packet = false;                     // the kernel's dispatch packet completes `end` (else a marker behind the kernel on the slot's stream)
  bool done_behind_counts = false;                // `done` is recorded on counts_stream behind the counts (else `end` is `done`)
};
SubmitRoute submit_route(const SubmitShape &in);
