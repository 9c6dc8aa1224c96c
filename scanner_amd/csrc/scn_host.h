// scn_host.h -- the C-ABI layer's arithmetic that never touches HIP (scn_host.hip).  Plain C++: tests/cpp/test_plan_math.cpp and
// tests/cpp/test_plan_resolve.cpp compile the unit with g++ and no HIP header on the include path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/scanner_hip.h"
#include "scn_mask.h"
#include "scn_sizes.h"

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
// A fused plan's ScnFftArgs::tw1_table, `rows` x `threads` (scn_tw1_layout / scn_mixed_layout): the values of twiddles<float>(n)
// regrouped per thread of the kernel, entry (p-1, t) = W_n^((stride t p) mod n)
std::vector<float> fused_tw1_table(uint32_t n, uint32_t rows, uint32_t threads, uint32_t stride = 1);
// What an averaged 8192-point plan reads besides: the tw1 table of the 4096-point transform of each half, [15][256], entry (p-1, t)
// = W_4096^(t p) = W_8192^((2 t p) mod 8192), and W_8192^k, k < 4096, in double (the radix-2 step that joins the halves)
struct ScnAvgHalfTables {
  std::vector<float> half;
  std::vector<double> join;
};
ScnAvgHalfTables avg_half_tables();

bool floor_permille_of(uint32_t given, uint32_t *permille);
uint32_t evaluated_bins(uint32_t n, uint32_t dc_ignore, double use_bandwidth, uint32_t *i_lo, uint32_t *i_hi);

// Everything of a plan that follows from its descriptor alone: resolve_plan applies the defaults, checks the descriptor and derives
// the rest, before scn_plan_create opens a device (tests/cpp/test_plan_resolve.cpp holds every field and every rejection).
struct PlanShape {
  scn_plan_desc d;  // with every default applied
  Path path = Path::Unsupported;
  uint32_t avg = 1, avg_layout = SCN_AVG_DWELL;  // scn_plan_desc.average / average_layout with the defaults applied
  size_t buf_bytes = 0;
  float scale = 1.0f;
  uint32_t i_lo = 0, i_hi = 0;
  uint32_t hit_region = 0;  // hit slots each buffer owns = the bins the mask of process.cpp:46-52 evaluates (cannot overflow)
  bool floor = false;       // scn_plan_desc.detect == SCN_DETECT_FLOOR: the transform stores the spectrum only, scn_floor.hip detects on it
  uint32_t floor_rank = 0;  // ... and the floor is the value of this rank among the hit_region evaluated bins
  uint32_t floor_permille = 0;  // ... (floor_permille with its default applied: what a floor window's ranks are made from)
  // scn_plan_desc.detect == SCN_DETECT_BASELINE: as a floor plan's, the transform stores the spectrum only and scn_baseline.hip detects
  // on it, against scn_plan::d_baseline
  bool baseline = false;
  // How the per-buffer counts reach the host.  false: a 4*n_buffers-byte copy on the d2h stream behind the kernel -- on
  // this ROCm a blit KERNEL, which runs beside the next launch when that leaves it room (up to 4096 points: yes, ~6 us)
  // and otherwise waits until that launch drains (8192 points: 254 VGPRs x 2 waves per SIMD; the copy took 46 us, the
  // host learned the counts late and submitted the launch after next ~10 us late, every other launch).  true: the FFT
  // kernel stores each count to pinned host memory as well (one 4-byte PCIe write per buffer; costs a 4096-point launch
  // ~4 us of completion latency, measured in round 1, and the 8192-point ones less than the late copy did).
  bool direct_counts = false;  // the fused kernels from 8192 points up
};
int resolve_plan(const scn_plan_desc *desc, PlanShape *out);  // SCN_OK, or the status with the error text set

// The same for a Welch plan (scn_welch_plan.hip)
struct WelchShape {
  scn_welch_desc d;  // with every default applied
  uint32_t hop = 0, bytes_per_sample = 0;
  float scale = 1.0f;  // K1's 1/max
  bool dc = false;     // correct_dc on an integer wire format
};
int resolve_welch(const scn_welch_desc *desc, WelchShape *out);
// workgroups that share the K segments of one PSD's row tile
uint32_t welch_parts(uint32_t max_psd, uint32_t segments_per_psd, int num_cus);
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

// The hit history (scanner_hip.h, "Hit history"): what a fold, a confirmation and a read-out must satisfy, from numbers alone (SCN_OK,
// or the status with the error text set) -- shared by the plan's entry points (scn_history_plan.hip) and the host forms
// (scn_history_fold_hits, scn_confirm_hits).  The row of a unit is scn_baseline_row, the mask and the predicate scn_history_mask and
// scn_history_confirms (scn_mask.h: the kernels' own).  rows: the history's; indexed: the submit named a run of the plan's table
int check_history_fold(uint32_t rows, uint32_t units, bool indexed, uint32_t table_count);
int check_history_window(uint32_t m, uint32_t window);
int check_history_range(uint32_t have, uint32_t first_row, uint32_t rows);

// The sweep trace (scanner_hip.h, "Sweep trace"): a geometry's limits and a read-out's range, from numbers alone -- shared by the
// plan's entry points (scn_trace_plan.hip) and the host forms (scn_trace_fold_spectrum, scn_trace_init, scn_trace_merge).  The
// arithmetic of a fold is scn_trace.h's, the kernel's own.
int check_trace_geometry(uint32_t cell_hz, uint32_t cells);
int check_trace_range(uint32_t have, uint32_t first_cell, uint32_t cells);
// The trace emitters (scanner_hip.h, "Trace emitters"): a line that exists and a threshold that is no NaN -- shared by the plan's entry
// point (scn_emitters_plan.hip) and the host form (scn_trace_emitters).  The arithmetic is scn_emitters.h's, the kernels' own.
int check_emitters_line(uint32_t line, float threshold_db);

// The level histogram (scanner_hip.h, "Level histogram"): a geometry's limits (the trace's, the number of edges, the words of the
// whole table), a table of edges -- no NaN, strictly increasing keys; keys: the kLevelsKeys padded keys of scn_levels.h, written
// only when the table is good -- and a summary's two numbers; shared by the plan's entry points (scn_levels_plan.hip) and the host
// forms.  The arithmetic is scn_levels.h's, the kernels' own.
int check_levels_geometry(uint32_t cell_hz, uint32_t cells, uint32_t n_edges);
int check_levels_edges(const float *edges_db, uint32_t n_edges, uint32_t *keys);
int check_levels_summary(uint32_t n_levels, uint32_t permille, uint32_t level);

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
  bool direct_counts;  // the plan's (PlanShape::direct_counts; fused plans only)
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
