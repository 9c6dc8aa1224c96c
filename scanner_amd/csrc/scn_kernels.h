// scn_kernels.h -- internal interface between the C-ABI layer (scn_plan.hip, scn_submit.hip,
// scn_collect.hip, scn_welch_plan.hip) and the
// kernel files (scn_kernels.hip, scn_mixed.hip, scn_average.hip, scn_big.hip, scn_generic.hip, scn_welch.hip, ...): argument structs and
// launchers.  K1's wire formats are scn_wire.h's (Wire<KIND>).  Not installed; the public surface is include/scanner_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_mask.h"  // scn_bin_evaluated: K5's mask, shared with the host arithmetic
#include "scn_sizes.h"  // scn_*_size_supported, scn_tw1_layout, scn_mixed_layout: which family takes a size, HIP-free
#include "scn_wire.h"  // SCN_K_*, scn_v2f, Wire<KIND>: K1's wire formats

typedef double double2_scn __attribute__((ext_vector_type(2)));

// A hit as the FFT kernel records it: slot `pos` of its buffer's region, in arbitrary order.  The compaction
// kernels (scn_hits.hip) put the batch's records into the order a single-threaded reference run prints them
// (buffer, then i: process.cpp:46-61) and complete them to the public scn_hit (seq_id, freq_hz).
struct ScnDevHit {
  uint32_t i;      // fftshift-ordered bin index (process.cpp:46)
  float power_db;  // magnitudes[j]
};

struct ScnFftArgs {
  const void *raw;          // n_buffers raw buffers back to back
  const float *window;      // [N]
  const scn_v2f *twiddle;   // W_N^m = exp(-2 pi i m / N), m in [0, N)
  const scn_v2f *tw1_table; // [15][N/16] ([31][512] for 16384 points, scn_tw1_layout): entry (p-1, t) = W_N^(t p): the pass-1 constants of thread t, p-major so that a
                            // wave loads each p with one coalesced 512-byte access (gathered from `twiddle` with lane
                            // stride 8p bytes the same 15 loads made the kernel prologue 6 us, up to 13 us, per launch)
  float *power_db;          // [n_buffers][N] or nullptr
  uint32_t n_buffers;
  float scale;              // onebymax of utility.cpp:65 (1.0 for float input)
  // K5 (process.cpp:46-62), all in the reference's uint32 arithmetic
  float threshold;
  float p_lo;               // pre-filter of the hit path in linear power: a shade below 10^(threshold / 5) (scn_hit_prefilter)
  uint32_t dc_ignore;       // m_dcIgnoreWindow
  uint32_t i_lo, i_hi;      // halfSampleCount -/+ m_useWindow (wrapping)
  // hit records: buffer b owns slots [b*hit_region, (b+1)*hit_region), hit_region = the number of bins the mask of
  // process.cpp:46-52 lets through, so a region can never overflow (sized for 288 GB of HBM: 8 B x ~0.75 N per
  // buffer, written only where there is a detection).  Slots are allocated with one LDS atomic per wave inside the
  // buffer's workgroup: no global atomics anywhere on the hit path.
  ScnDevHit *hits;            // [n_buffers][hit_region]
  uint32_t hit_region;
  uint32_t *per_buffer_hits;  // [n_buffers] total hits of each buffer (device memory)
  uint32_t *host_hits;        // optional second copy of the same counts in pinned HOST memory, written by the kernel (see
                              // PlanShape::direct_counts in scn_host.h for when that beats a copy behind the kernel)
  // buffer queue of the persistent workgroups: 8 heads, 32 words (one 128-byte line) apart, never reset; head x
  // serves the buffers b = 8 j + x; work_base[x] is its value before this launch and a launch adds exactly the
  // number of such buffers (scn_work_shard_count) to it
  uint32_t *work_counter;
  uint32_t work_base[8];
};
// which wire formats pull their buffers from the queue (the compute-bound integer ones; the float path is
// memory-bound and measurably better off with the static assignment)
// ... and only from 4096 points up: a launch of the same sample count makes 4x / 2x as many dequeues at 1024 / 2048
// points, and the queue heads then become the bottleneck (1024-pt int16: 64.7 us static, 90.7 us with the queue)
static constexpr bool scn_uses_queue(int kind, uint32_t n) {
  return kind != SCN_K_FLOAT_COMPLEX && n >= 4096 && n <= 8192;  // (16384: static, one workgroup per CU)
}
// number of buffers b < n_buffers with b % 8 == shard
static inline uint32_t scn_work_shard_count(uint32_t n_buffers, uint32_t shard) {
  return n_buffers > shard ? (n_buffers - shard + 7u) / 8u : 0u;
}

// time-domain mode (process.cpp:203-237)
struct ScnTdArgs {
  const void *raw;
  uint32_t n, n_buffers;
  float scale;
  float *max_db;  // [n_buffers] pinned host memory
  float *min_db;
};
hipError_t scn_launch_time_domain(int kind, bool correct_dc, const ScnTdArgs &args, int num_cus, hipStream_t stream);

// Welch PSD (BASELINE C5): 65 536-pt four-step FFT, 50 % overlap, K-segment power average
struct ScnWelchArgs {
  const void *in;          // the stream in the plan's wire format, (n_psd*k + 1) delivery blocks of hop samples
  const float *window;     // [65536]
  const scn_v2f *twiddle;  // W_65536^m
  void *work;              // [n_segments][65536] complex: Y[k1][n2] between the two kernels
  float *psd_db;           // [n_psd][65536]
  float *partial;          // [parts][n_psd][65536] partial |X|^2 sums between the row and the combine kernel
  uint32_t n_segments, hop, k, n_psd;
  uint32_t parts;          // workgroups that share the K segments of one PSD row tile (1: no combine kernel)
  float inv_k;
  float scale;             // K1's 1/max (utility.cpp:16-17,40-41,64-65); 1 for float samples
  int *dc_sums;            // [n_segments + 1][2] integer sums per delivery block (correctDC on integer samples), or nullptr
  const double2_scn *tw256;  // W_256^m, m in [0, 256), in double: the row transform's twiddles
};
hipError_t scn_launch_welch(int kind, bool correct_dc, const ScnWelchArgs &args, int num_cus, hipStream_t stream);
// the column kernel's split of a submit: `groups` workgroups per column tile, `per` consecutive segments each (the last ragged)
void scn_welch_column_groups(uint32_t n_segments, int num_cus, uint32_t *groups, uint32_t *per);

// Ordered hit list (scn_hits.hip): exclusive scan of the per-buffer counts, then one wave per buffer with hits ranks
// its records by bin (a bitmap in LDS) and writes the completed scn_hit records [first, first + out_cap) of the
// batch's ordered list to `out` (device or pinned host memory).
struct ScnCompactArgs {
  const ScnDevHit *regions;  // [n_buffers][hit_region]
  uint32_t hit_region;
  const uint32_t *counts;    // [n_buffers]
  uint32_t *offsets;         // [n_buffers + 1]: exclusive prefix sums, total at [n_buffers]
  const double *center_freq; // [n_buffers] the submit's MessageHeader fields, read IN PLACE from the plan's pinned host
  const uint64_t *seq_id;    // [n_buffers] copy (two 8-byte reads per buffer that has hits: no staging copies on the stream)
  uint32_t table_count;      // 0: center_freq is the submit's own [n_buffers]; else center_freq is the plan's device-resident frequency
  uint32_t table_first;      //    table and buffer b carries entry (table_first + b) % table_count (scn_submit*_indexed)
  void *out;                 // scn_hit[out_cap]
  uint32_t first, out_cap;
  uint32_t n_buffers, n, sample_rate;
};
hipError_t scn_launch_hit_scan(const ScnCompactArgs &args, hipStream_t stream);
hipError_t scn_launch_hit_compact(const ScnCompactArgs &args, hipStream_t stream);
// Signals (scn_hits.hip): the units' hits, where the FFT kernels and the scan above left them, merged into one scn_signal per run
// of hits no more than max_gap non-hit bins apart.  scn_launch_signal_count writes each unit's number of signals,
// scn_launch_hit_scan (counts = sig_counts, offsets = sig_offsets) turns them into offsets and the total, and
// scn_launch_signal_build writes the records [first, first + out_cap) of the batch's ordered signal list to `out`.
struct ScnSignalArgs {
  const ScnDevHit *regions;    // as ScnCompactArgs: regions, the hits' offsets (the scan's output) and the submit's header fields
  uint32_t hit_region;
  const uint32_t *offsets;     // [n_buffers + 1]
  const double *center_freq;
  const uint64_t *seq_id;
  uint32_t table_count, table_first;
  uint32_t n_buffers, n, sample_rate;
  uint32_t max_gap;
  uint32_t *sig_counts;        // [n_buffers] signals per unit (the count kernel's output)
  const uint32_t *sig_offsets; // [n_buffers + 1] their exclusive prefix sums, the total last (the build kernel's input)
  void *out;                   // scn_signal[out_cap]
  uint32_t first, out_cap;     // first + out_cap must not wrap
  uint32_t map_words, chunk, wave_words;  // LDS layout per wave, filled in by the launchers
};
hipError_t scn_launch_signal_count(const ScnSignalArgs &args, hipStream_t stream);
hipError_t scn_launch_signal_build(const ScnSignalArgs &args, hipStream_t stream);
// The hit history (scn_history.hip, scanner_hip.h "Hit history"): history[rows][n] words by fftshift index and visits[rows], device
// memory, per plan.  The fold launch shifts a submit's hits -- the units' regions and counts where the FFT kernels and the detectors
// left them, in any order -- into the rows of its units, every bin of each row: word = (word << 1) | hit, and adds one to each such
// row's visits (saturating).  It needs n_units <= rows: every unit then has a row of its own, no two threads write the same word.
struct ScnHistoryArgs {
  const ScnDevHit *regions;    // [n_units][hit_region]
  uint32_t hit_region;
  const uint32_t *counts;      // [n_units] hits per unit
  uint32_t *history;           // [rows][n]
  uint32_t *visits;            // [rows]
  uint32_t n, n_units;
  uint32_t rows, first;        // unit u folds into row scn_baseline_row(first, u, rows); first < rows
};
hipError_t scn_launch_history_fold(const ScnHistoryArgs &args, int num_cus, hipStream_t stream);
// The confirmed list: the records of the submit's ordered hit list whose history word has at least m of the bits of `mask` set
// (scn_history_confirms), in the list's order.  scn_launch_confirm_count writes each unit's number of confirmed records,
// scn_launch_hit_scan (counts = conf_counts, offsets = conf_offsets) turns them into offsets and the total, and
// scn_launch_confirm_build writes the completed records [first, first + out_cap) of the confirmed list to `out`.
struct ScnConfirmArgs {
  const ScnDevHit *regions;    // as ScnSignalArgs: regions, the hits' offsets (the scan's output) and the submit's header fields
  uint32_t hit_region;
  const uint32_t *offsets;     // [n_buffers + 1]
  const double *center_freq;
  const uint64_t *seq_id;
  uint32_t table_count, table_first;
  uint32_t n_buffers, n, sample_rate;
  const uint32_t *history;     // [rows][n]
  uint32_t rows, hist_first;   // unit b reads row scn_baseline_row(hist_first, b, rows); hist_first < rows
  uint32_t m, mask;            // scn_history_mask(window)
  uint32_t *conf_counts;       // [n_buffers] confirmed records per unit (the count kernel's output)
  const uint32_t *conf_offsets;  // [n_buffers + 1] their exclusive prefix sums, the total last (the build kernel's input)
  void *out;                   // scn_hit[out_cap]
  uint32_t first, out_cap;     // first + out_cap must not wrap
};
hipError_t scn_launch_confirm_count(const ScnConfirmArgs &args, hipStream_t stream);
hipError_t scn_launch_confirm_build(const ScnConfirmArgs &args, hipStream_t stream);
// The sweep trace (scn_trace.hip, scanner_hip.h "Sweep trace"): per cell of the plan's frequency grid the largest and the smallest
// dB value folded into it, as ordered keys (scn_trace.h), and their number.  The fold launch reads the spectrum a collected submit
// stored and its centres where the submit left them, and changes the three arrays with atomics only: any number of units may name
// the same cell.
struct ScnTraceArgs {
  const float *power_db;       // [n_units][n], natural bin order
  const double *center_freq;   // as ScnCompactArgs: the submit's own [n_units], or the plan's table
  uint32_t table_count, table_first;
  uint32_t n, n_units, sample_rate;
  uint32_t dc_ignore, i_lo, i_hi;
  uint64_t f0_hz;              // the grid: cell c covers [f0_hz + c cell_hz, f0_hz + (c + 1) cell_hz)
  uint32_t cell_hz, cells;     // cell_hz >= 1, 1 <= cells <= SCN_TRACE_CELLS_MAX
  uint32_t *max_key, *min_key; // [cells] scn_trace_key of max_db / min_db (empty: kTraceEmptyMaxKey / kTraceEmptyMinKey)
  unsigned long long *count;   // [cells]
};
hipError_t scn_launch_trace_fold(const ScnTraceArgs &args, int num_cus, hipStream_t stream);
// The level histogram (scn_levels.hip, scanner_hip.h "Level histogram"): per cell of the plan's frequency grid and per level of its
// table of edges, how many dB values were folded into it.  The fold launch reads what the trace's reads (the same fields under the
// same names) and changes the counters with atomics only; the summary launch reduces cells [first_cell, first_cell + cells) to
// three numbers each.
struct ScnLevelsArgs {
  const float *power_db;       // [n_units][n], natural bin order
  const double *center_freq;   // as ScnTraceArgs
  uint32_t table_count, table_first;
  uint32_t n, n_units, sample_rate;
  uint32_t dc_ignore, i_lo, i_hi;
  uint64_t f0_hz;              // the grid, as the trace's
  uint32_t cell_hz, cells;
  const uint32_t *edge_keys;   // [kLevelsKeys] the edges' keys, padded (scn_levels.h)
  uint32_t n_edges;            // 1 ... SCN_LEVELS_EDGES_MAX; cells * (n_edges + 1) <= SCN_LEVELS_WORDS_MAX
  unsigned long long *hist;    // [cells][n_edges + 1]
};
hipError_t scn_launch_levels_fold(const ScnLevelsArgs &args, int num_cus, hipStream_t stream);
struct ScnLevelsSummaryArgs {
  const unsigned long long *hist;  // [..][n_levels]
  uint32_t first_cell, cells, n_levels;
  uint32_t permille, level;        // permille <= 1000, level < n_levels
  uint32_t *rank_level;            // [cells] each
  unsigned long long *above, *total;
};
hipError_t scn_launch_levels_summary(const ScnLevelsSummaryArgs &args, hipStream_t stream);
// The trace emitters (scn_emitters.hip, scanner_hip.h "Trace emitters"): a window of the plan's trace segmented into runs of on cells,
// one record per run.  Three launches on one stream: scn_launch_emitters_count leaves *total and the tiles' carries; the caller reads
// *total, zeroes acc[0, total) and then has scn_launch_emitters_build gather every emitter into acc (integer atomics only) and
// scn_launch_emitters_finish turn acc[first, first + out_cap) into records.  kEmitTile: the cells of a tile, one wave's.
constexpr uint32_t kEmitTile = 1024;
constexpr uint32_t kEmitTilesMax = (1u << 22) / kEmitTile;  // SCN_TRACE_CELLS_MAX's (static_assert: scn_emitters.hip)
struct ScnEmitterAcc {         // what the build pass gathers of one emitter; all zero before it
  unsigned long long key;      // scn_emit_peak_key of the peak (atomicMax)
  unsigned long long count;    // sum over the on cells (atomicAdd)
  uint32_t first_cell;         // stored by the emitter's first cell alone
  uint32_t last_cell;          // atomicMax
  uint32_t n_cells;            // atomicAdd
  uint32_t reserved;
};
struct ScnEmittersArgs {
  const uint32_t *max_key, *min_key;  // the plan's trace, cell 0 first (keys: scn_trace.h)
  const unsigned long long *count;
  uint64_t f0_hz;
  uint32_t cell_hz;
  uint32_t first_cell, cells;  // the window; cells >= 1, first_cell + cells <= the trace's cells
  uint32_t line, threshold_bits, max_gap;
  // per tile t of the window, [kEmitTilesMax] each.  The count pass: the tile's last on cell + 1 (0: none), its first on cell, its
  // starts with its first on cell counted as one.  Its scan: the last on cell + 1 before the tile, the starts before the tile.
  uint32_t *tile_last, *tile_first, *tile_starts, *carry_last, *carry_starts;
  uint32_t *total;             // [1] emitters of the window
  ScnEmitterAcc *acc;          // [acc_cap], acc_cap >= *total
  uint32_t acc_cap;
  void *out;                   // scn_emitter[out_cap]: records [first, first + out_cap), first + out_cap <= *total
  uint32_t first, out_cap;
};
hipError_t scn_launch_emitters_count(const ScnEmittersArgs &args, hipStream_t stream);
hipError_t scn_launch_emitters_build(const ScnEmittersArgs &args, hipStream_t stream);
hipError_t scn_launch_emitters_finish(const ScnEmittersArgs &args, hipStream_t stream);
// scn_trace_merge on the device: cells [first_cell, first_cell + cells) of the trace take in src (float bits and counts, no NaN)
struct ScnTraceMergeArgs {
  uint32_t *max_key, *min_key;  // the plan's trace, cell 0 first
  unsigned long long *count;
  uint32_t first_cell, cells;
  const uint32_t *src_max, *src_min;  // [cells] float bits
  const unsigned long long *src_count;
};
hipError_t scn_launch_trace_merge(const ScnTraceMergeArgs &args, hipStream_t stream);
// sum of counts[0, n_buffers) -> *host_total (pinned host memory); acc: two zeroed device words the kernel leaves zeroed
hipError_t scn_launch_hit_total(const uint32_t *counts, uint32_t n_buffers, uint32_t trigger_count, unsigned long long *acc, unsigned long long *host_total,
                                uint32_t *trigger_bits, hipStream_t stream);

// The floor detector (scn_floor.hip, scn_plan_desc.detect = SCN_DETECT_FLOOR): behind the transform, on the dB spectrum it stored.
// Per unit: the value of rank `rank` among the evaluated bins (floor_db[u]), the cut floor_db[u] + threshold in one float
// addition, and every evaluated bin strictly above the cut as a record of the unit's region, with the unit's count -- regions and
// counts as the FFT kernels' hit paths leave them.  Every unit's count and floor are written (nothing to zero beforehand).
struct ScnFloorArgs {
  const float *power_db;      // [n_units][n], natural bin order
  uint32_t n, n_units;
  uint32_t rank;              // floor_permille * (hit_region - 1) / 1000, < hit_region
  float threshold;            // the offset above the floor, in the plan's dB scale
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_units][hit_region]
  uint32_t hit_region;        // = the number of evaluated bins M
  uint32_t *counts;           // [n_units]
  float *floor_db;            // [n_units] (device memory)
};
hipError_t scn_launch_floor(const ScnFloorArgs &args, int num_cus, hipStream_t stream);

// The floor detector with a floor window (scn_floor_local.hip, scn_plan_set_floor_window): the same place behind the transform, the
// same regions and counts; bin i of a unit is a hit iff at least need[i] of its reference cells c have c + threshold < power_db --
// the order-statistic cut without a selection.  Every unit's count is written (nothing to zero beforehand); there is no per-unit floor.
struct ScnFloorLocalArgs {
  const float *power_db;      // [n_units][n], natural bin order
  uint32_t n, n_units;
  uint32_t train, guard;      // 1 <= train <= SCN_FLOOR_TRAIN_MAX, guard <= SCN_FLOOR_GUARD_MAX
  uint32_t permille;          // what `need` was made with (floor_window_ranks); the kernel reads the table
  const uint16_t *need;       // [n] by fftshift index i: r_i + 1 for an evaluated bin, 0 for the others (device memory, per plan)
  float threshold;            // the offset above the floor, in the plan's dB scale
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_units][hit_region]
  uint32_t hit_region;        // = the number of evaluated bins M
  uint32_t *counts;           // [n_units]
};
hipError_t scn_launch_floor_local(const ScnFloorLocalArgs &args, int num_cus, hipStream_t stream);

// The baseline detector (scn_baseline.hip, scn_plan_desc.detect = SCN_DETECT_BASELINE): the same place behind the transform, the same
// regions and counts; bin j of unit u is a hit iff power_db[u][j] > baseline_db[row][j] + threshold, row = scn_baseline_row(first, u,
// rows).  The detect launch only reads the baseline and writes every unit's count (nothing to zero beforehand).  The update launch
// (scn_plan_update_baseline) reads the same spectra and writes the same rows, all n bins of each: op SCN_BASELINE_SET copies the
// bits, SCN_BASELINE_MAX keeps the larger in the floor's key order; it needs n_units <= rows and reads none of the hit fields.
struct ScnBaselineArgs {
  const float *power_db;      // [n_units][n], natural bin order
  float *baseline_db;         // [rows][n], natural bin order (device memory, per plan)
  uint32_t n, n_units;
  uint32_t rows, first;       // first < rows
  float threshold;            // the offset above the baseline, in the plan's dB scale
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_units][hit_region]
  uint32_t hit_region;        // = the number of evaluated bins M
  uint32_t *counts;           // [n_units]
  uint32_t op;                // the update launch: SCN_BASELINE_SET / SCN_BASELINE_MAX
};
hipError_t scn_launch_baseline_detect(const ScnBaselineArgs &args, int num_cus, hipStream_t stream);
hipError_t scn_launch_baseline_update(const ScnBaselineArgs &args, hipStream_t stream);

// The same path for the sizes without a fused or four-step kernel (scn_generic.hip): Bluestein, through HBM, stage by stage
struct ScnGenericArgs {
  const void *raw;            // n_buffers raw buffers back to back
  const float *window;        // [n]
  const void *twiddle;        // double[m][2]: W_m^k, k in [0, m): the table of the TRANSFORM length, in double
  void *work0, *work1;        // double[n_buffers][m][2] each: ping-pong between the stages
  float *power_db;            // [n_buffers][n] or nullptr
  uint32_t n, n_buffers;      // buffer length (samples, bins)
  uint32_t m, log2m;          // transform length: the power of two >= 2n - 1
  const void *chirp;          // double[n][2], w[i] = exp(-i pi i^2 / n)
  const void *bfilter;        // double[m][2], FFT_m of the chirp filter, scaled by 1/m
  float scale, threshold;
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_buffers][hit_region]
  uint32_t hit_region;
  uint32_t *per_buffer_hits;  // [n_buffers], zeroed by the launcher
};
hipError_t scn_launch_generic(int kind, bool correct_dc, bool hits, const ScnGenericArgs &args, int num_cus, hipStream_t stream);

// Plain 65536- / 32768-point plans through the four-step pair of scn_big.hip (columns -> tiled work buffer -> rows + K4 + K5)
struct ScnBigArgs {
  const void *raw;            // n_buffers raw buffers back to back
  const float *window;        // [65536]
  const scn_v2f *twiddle;     // W_65536^m
  void *work;                 // [n_buffers][65536] complex float: Y[k1][n2] between the two kernels (tiled)
  const double2_scn *tw256;   // W_256^m, m in [0, 256), in double: the row transform's twiddles
  float *power_db;            // [n_buffers][65536] or nullptr
  uint32_t n_buffers;
  float scale, threshold, p_lo;
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_buffers][hit_region]
  uint32_t hit_region;
  uint32_t *per_buffer_hits;  // [n_buffers], zeroed by the column kernel (tile 0), counted into by the row kernel
  int *dc_sums;               // [n_buffers][2] scratch for DC removal of integer samples (zeroed by the launcher), or nullptr
};
hipError_t scn_launch_big(uint32_t n, int kind, bool correct_dc, bool hits, bool spectrum, const ScnBigArgs &args, int num_cus, hipStream_t stream);

// Averaged plans (scn_average.hip, scn_plan_desc.average = K > 1): n_groups groups of k buffers, each buffer through K1 + K2 +
// K3 as in the fused kernels, the group's powers summed in float, divided by k, then K4 + K5 once per group
#define SCN_AVG_L_DWELL 0   // buffers g k ... g k + k - 1 (SCN_AVG_DWELL)
#define SCN_AVG_L_SWEEPS 1  // buffers g, g + n_groups, ... (SCN_AVG_SWEEPS)
struct ScnAvgArgs {
  const void *raw;            // n_groups * k raw buffers back to back
  const float *window;        // [n]
  const scn_v2f *twiddle;     // W_n^m
  const scn_v2f *tw1_table;   // as ScnFftArgs::tw1_table (1024 ... 4096 points)
  const scn_v2f *tw1_half;    // 8192 points: the same table of the 4096-point transform of each half, [15][256]
  const double2_scn *tw_half; // 8192 points: W_8192^k, k < 4096, in double (the radix-2 step that joins the halves)
  float *partial;             // [n_groups][parts][n] linear power sums of the parts (between the two kernels)
  float *power_db;            // [n_groups][n] or nullptr
  uint32_t n, n_groups, k, parts, layout;
  float scale, threshold, p_lo;
  uint32_t dc_ignore, i_lo, i_hi;
  ScnDevHit *hits;            // [n_groups][hit_region]
  uint32_t hit_region;
  uint32_t *per_group_hits;   // [n_groups], zeroed by the launcher
};
// workgroups that share the k buffers of one group (1 <= parts <= max(1, ceil(k / 2)))
uint32_t scn_avg_parts(uint32_t n, uint32_t n_groups, uint32_t k, int num_cus);
// floats of the partial-sum buffer a launch of up to max_groups groups needs
size_t scn_avg_partial_floats(uint32_t n, uint32_t max_groups, int num_cus);
hipError_t scn_launch_average(int kind, bool correct_dc, bool hits, bool spectrum, const ScnAvgArgs &args, int num_cus, hipStream_t stream);

// K1 alone (capture path)
hipError_t scn_launch_convert(int kind, bool correct_dc, const void *raw, scn_v2f *out, uint32_t n, uint32_t n_buffers,
                              float scale, hipStream_t stream);

// hits / spectrum: what the launch reports (at least one).  hits && !spectrum runs the hits-only kernels: no stores, no
// per-bin logarithm.
hipError_t scn_launch_fft(uint32_t n, int kind, bool correct_dc, bool hits, bool spectrum, const ScnFftArgs &args,
                          int num_cus, hipStream_t stream, hipEvent_t stop = nullptr);
// The linear-power pre-filter that goes with a dB threshold: every power whose dB value (the map of scn_device.h, error
// <= 2.2 ulp) can exceed `threshold` is > the returned value.  NaN -> NaN (nothing passes), +inf -> +inf.
static inline float scn_hit_prefilter(float threshold) {
  if (!(threshold == threshold)) return threshold;
  const double t = (double)threshold, guard = 1e-6 * (t < 0 ? -t : t) + 1e-5;
  const double p = __builtin_pow(10.0, (t - guard) / 5.0);
  float f = (float)p;
  if ((double)f > p) f = __builtin_nextafterf(f, 0.0f);
  return f;
}
// a fused launch on its way from scn_launch_fft / scn_launch_mixed to the translation unit that holds the size's kernels
struct ScnFftLaunch {
  int kind;
  bool dc, hits, spec;
  const ScnFftArgs &args;
  int num_cus;
  hipStream_t stream;
  hipEvent_t stop;
};

// The fused kernels for the sizes 2^a 3^b 5^c that are not powers of two (scn_mixed.hip, scn_mixed_plans.h): same arguments, same
// outputs.  tw1_table: `rows` rows of `threads` entries, entry (p - 1, t) = W_n^(t p) (scn_mixed_layout); twiddle: W_n^m, m < n.
hipError_t scn_launch_mixed(uint32_t n, int kind, bool correct_dc, bool hits, bool spectrum, const ScnFftArgs &args, int num_cus,
                            hipStream_t stream, hipEvent_t stop = nullptr);
