/*
 * scanner_hip.h -- C-ABI of the MI355X spectrum-scan DSP path.
 *
 * The reference (wpats/scanner) has no FFI: its boundary is the C++ class
 * surface ProcessSamples / SampleQueue.  This header is the cut just below
 * those classes and just above the arithmetic: one `scn_plan` replaces what
 * one consumer thread of the reference owns (process.cpp:101-107: per-thread
 * input/output buffers, the FFT plan of fft.cpp:4-11, the window of
 * process.cpp:14-21) plus the producer-side convert of
 * messageQueue.h:190-237, batched over many buffers per submit.
 *
 * Conventions: every entry point returns an int status (SCN_OK == 0); nothing
 * exits or throws across the boundary (the reference's device layers exit(1),
 * e.g. hackRFSource.cpp:19-30 -- a library must not).  All pointers are plain
 * host or device addresses; no C++ or torch types.  A plan is NOT thread-safe
 * and owns one HIP stream: use one plan per consumer thread, as the reference
 * uses one buffer set per thread.  Different plans may run concurrently.
 */
#ifndef SCANNER_HIP_H
#define SCANNER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Marks the entry points: the ONLY symbols the shared library exports (it is built with hidden visibility and a version
 * script generated from these declarations).  Expands to nothing in a caller's translation unit. */
#if defined(SCN_BUILDING_LIBRARY)
#define SCN_API __attribute__((visibility("default")))
#else
#define SCN_API
#endif

#define SCN_ABI_VERSION 6 /* 3: SCN_NUM_SLOTS 4, scn_gather_hits_device, scn_gather_fetch, scn_size_path; 4: scn_plan_set_table, scn_submit*_indexed;
                             5: scn_welch_desc.sample_kind / enob / correct_dc (carved out of its reserved words: same size, zero = the
                             version-4 behaviour), scn_welch_partition, scn_gather_post, scn_gather_wait;
                             6: scn_plan_desc.average / average_layout (carved out of its reserved words: same size, zero = the
                             version-5 behaviour), SCN_AVG_*, scn_plan_average_parts;
                             still 6 (additions only, nothing existing changes): scn_signal, scn_collect_signals,
                             scn_signals_from_hits; scn_plan_desc.detect / floor_permille (carved out of its reserved words: same
                             size, zero = the fixed threshold), SCN_DETECT_*, SCN_FLOOR_MIN, scn_collect_floor,
                             scn_floor_from_spectrum;
                             still 6 (additions only): the floor window -- SCN_FLOOR_TRAIN_MAX, SCN_FLOOR_GUARD_MAX,
                             scn_plan_set_floor_window, scn_local_floor_from_spectrum;
                             still 6 (additions only): the baseline detector -- SCN_DETECT_BASELINE, SCN_BASELINE_*,
                             scn_plan_set_baseline, scn_plan_update_baseline, scn_plan_get_baseline;
                             still 6 (additions only): the hit history -- scn_plan_set_history, scn_plan_update_history,
                             scn_plan_get_history, scn_collect_confirmed, scn_history_fold_hits, scn_confirm_hits;
                             still 6 (additions only): the sweep trace -- SCN_TRACE_CELLS_MAX, scn_plan_set_trace,
                             scn_plan_update_trace, scn_plan_get_trace, scn_trace_fold_spectrum, scn_trace_init, scn_trace_merge;
                             still 6 (additions only): the level histogram -- SCN_LEVELS_EDGES_MAX, SCN_LEVELS_WORDS_MAX,
                             scn_plan_set_levels, scn_plan_update_levels, scn_plan_get_levels, scn_plan_levels_summary,
                             scn_levels_fold_spectrum, scn_levels_merge, scn_levels_summary;
                             still 6 (additions only): the trace emitters -- SCN_TRACE_LINE_*, scn_emitter, scn_trace_emitters,
                             scn_plan_trace_emitters, scn_plan_merge_trace */

/* status codes */
enum {
  SCN_OK = 0,
  SCN_E_INVALID = 1,      /* bad argument / unsupported configuration */
  SCN_E_HIP = 2,          /* a HIP runtime call failed (see scn_last_error) */
  SCN_E_NOMEM = 3,
  SCN_E_STATE = 4,        /* call out of order (collect before submit, ...) */
  SCN_E_TRUNCATED = 5,    /* more hits than the caller's buffer (or the plan's max_hits) holds: n_hits is the true
                             total, the buffer holds the FIRST min(n_hits, hit_cap, max_hits) records of the ordered
                             list and nothing is lost on the GPU: scn_collect_more fetches the rest */
  SCN_E_NO_DEVICE = 6,
  SCN_E_COMM = 7          /* RCCL could not be loaded or a collective failed */
};

/* Wire format of one IQ sample; values are messageQueue.h:31-37 SampleKind. */
enum {
  SCN_KIND_BYTE_COMPLEX = 1,  /* int8  I,Q interleaved (hackRFSource.cpp:261) */
  SCN_KIND_SHORT = 2,         /* int16 planar: I[n] then Q[n] (sdrplaySource.cpp:197) */
  SCN_KIND_SHORT_COMPLEX = 3, /* int16 I,Q interleaved (bladerfSource.cpp:297) */
  SCN_KIND_FLOAT_COMPLEX = 4  /* float I,Q interleaved (airspySource.cpp:197) */
};

/* process.h:27-31 ProcessSamples::Mode */
enum { SCN_MODE_TIME_DOMAIN = 1, SCN_MODE_FREQUENCY_DOMAIN = 2 };

/* gr::fft::window::win_type (GNU Radio 3.7 / 3.8 numbering), what process.cpp:18 hands to window::build(type, N, 0.0): every
 * type is built ([3P] published definitions; scan.cpp:215 only ever passes Blackman-Harris).  One exception to the numbering:
 * 0 is WIN_HAMMING there and "the default" in the zero-initialised descriptors here, so Hamming travels as 8. */
enum {
  SCN_WIN_HANN = 1,
  SCN_WIN_BLACKMAN = 2,
  SCN_WIN_RECTANGULAR = 3,
  SCN_WIN_KAISER = 4, /* with the beta the reference passes, 0.0: all ones */
  SCN_WIN_BLACKMAN_HARRIS = 5,
  SCN_WIN_BARTLETT = 6,
  SCN_WIN_FLATTOP = 7,
  SCN_WIN_HAMMING = 8
};

/* output selection (flags) */
enum {
  SCN_OUT_SPECTRUM = 1u, /* keep the N-bin dB spectrum of every buffer */
  SCN_OUT_HITS = 2u,     /* threshold every in-band bin into the hit list.  Alone (no SCN_OUT_SPECTRUM): the hits-only
                          * kernels -- no spectrum is stored and no per-bin logarithm taken; the same bins are reported,
                          * with the same power_db, as with the spectrum kept */
  /* Not an output: give each slot its own compute stream, so that the launch of one slot
   * overlaps the tail of the other slot's launch (the next batch's workgroups fill the CUs the finishing
   * batch frees) instead of waiting for it to drain.  Measured on C2: one launch per 67.6 us instead of
   * 76.0 (+12 % throughput).  Off by default because each kernel's own begin-to-end time grows while it
   * shares the GPU with its neighbour, which is what per-kernel profiles and bench.py's roofline accounting
   * divide by; results are identical either way (the slots share nothing but read-only tables).
   * With it, scn_plan_stream returns slot 0's stream and scn_slot_stream each slot's. */
  SCN_PLAN_OVERLAP_SLOTS = 4u
};

/* One detection: a `freq %lu power_db %f` line of process.cpp:57. */
typedef struct scn_hit {
  uint64_t seq_id;  /* MessageHeader::m_sequenceId of the buffer */
  uint32_t i;       /* fftshift-ordered bin index, the loop variable of process.cpp:46 */
  float power_db;   /* magnitudes[j], j = (i + N/2) % N */
  uint64_t freq_hz; /* uint64_t(start_frequency + i*bin_step), process.cpp:55-57 */
} scn_hit;

/* Everything the reference bakes into the ProcessSamples (process.h:74-85) and
 * SampleQueue (messageQueue.h:141-146) constructors.  Zero-initialise, set
 * struct_size = sizeof(scn_plan_desc), then fill; 0 picks the reference's
 * constant where one exists. */
typedef struct scn_plan_desc {
  uint32_t struct_size;
  uint32_t n;              /* sampleCount = FFT size (scan.cpp:85; the reference plans any count, fft.cpp:4-11): any size from
                              16 to 65536.  The powers of two from 16 to 16384 run in fused single-pass LDS kernels, 32768
                              and 65536 in a four-step pair of kernels (integer DC removal included); the sizes that are
                              not powers of two through a staged, slower path (Bluestein, in double) with the same outputs.
                              scn_size_path tells which. */
  uint32_t sample_rate;    /* Hz (scan.cpp:92) */
  uint32_t sample_kind;    /* SCN_KIND_* */
  uint32_t enob;           /* effective bits (scan.cpp:138,183) */
  uint32_t correct_dc;     /* SampleQueue correctDCOffset */
  uint32_t window_type;    /* 0 -> SCN_WIN_BLACKMAN_HARRIS */
  uint32_t mode;           /* 0 -> SCN_MODE_FREQUENCY_DOMAIN; SCN_MODE_TIME_DOMAIN accepts any n >= 1 */
  float threshold;         /* dB (scan.cpp:94) */
  uint32_t dc_ignore_bins; /* 0 -> 4 (process.cpp:87); use SCN_DC_IGNORE_NONE for none */
  double use_bandwidth;    /* 0 -> 0.75 (scan.cpp:65) */
  uint32_t trigger_count;  /* 0 -> 1047 (process.cpp:62) */
  uint32_t max_batch;      /* buffers per submit (>= 1) */
  uint32_t max_hits;       /* records of the ordered hit list each slot keeps in pinned host memory (what one
                              scn_collect can return; the rest stays on the GPU for scn_collect_more); 0 -> 64 per buffer */
  uint32_t flags;          /* SCN_OUT_* (neither -> SPECTRUM|HITS), SCN_PLAN_OVERLAP_SLOTS */
  int32_t device_id;       /* HIP device ordinal */
  uint32_t average;        /* 0 -> 1.  K > 1: average K buffers per centre frequency before detection (below) */
  uint32_t average_layout; /* 0 -> SCN_AVG_DWELL: which buffers of a submit form a group */
  uint32_t detect;         /* SCN_DETECT_*; 0 -> SCN_DETECT_FIXED: power_db > threshold */
  uint32_t floor_permille; /* SCN_DETECT_FLOOR only: the rank of the floor among the evaluated bins, in permille (below) */
  uint32_t reserved[1];
} scn_plan_desc;

/* Averaged plans (average = K > 1; Bartlett's method: no overlap, whole buffers).  A submit of n_buffers = K*G buffers forms G
 * groups of K buffers.  Every buffer goes through convert (with its own DC removal), window and FFT exactly as in a plain plan;
 * the group's spectrum is 5*log10(P[j]), P[j] = (sum over the group's buffers, in order, of |X_b[j]|^2) / (float)K, and the
 * mask, threshold, records and trigger run on it ONCE per group with the group's centre frequency.  So every output is per
 * group: power_db / d_power_db / scn_device_spectrum hold G*N floats, trigger G bytes, and the ordered hit list is ordered by
 * (group, i); a record's seq_id is that of the group's FIRST buffer (its seq_ids entry, or its index when seq_ids is NULL).
 * Frequency-domain plans of 1024, 2048, 4096 and 8192 points only (other sizes, time-domain mode, a max_batch that is not a
 * multiple of K and an unknown layout: SCN_E_INVALID at create).  A submit with n_buffers % K != 0 is SCN_E_INVALID; so is one whose
 * center_freqs (still one per buffer) differ inside a group.  Indexed submits: group g carries
 * center_freqs[(first_index + g) % count] of the plan's table.  When G is small the K buffers of a group are split over
 * several workgroups whose partial sums are added in a fixed order (scn_plan_average_parts): results are deterministic, but
 * with more than one part the float sum is grouped differently from a single running sum.  K = 1 is the plain plan. */
enum {
  SCN_AVG_DWELL = 0,  /* group g = buffers g*K ... g*K + K - 1: K buffers of one centre back to back (a dwell) */
  SCN_AVG_SWEEPS = 1  /* group g = buffers g, g + G, ..., g + (K-1)*G: K whole sweeps of a G-centre table back to back */
};

/* Floor detector (detect = SCN_DETECT_FLOOR): the threshold rides on each unit's own noise floor.  A unit is a buffer (for an
 * averaged plan: the group).  For a unit u let E be the natural bins j the mask of process.cpp:46-52 lets through (M = |E| > 0; a
 * plan whose mask lets no bin through is SCN_E_INVALID at create).  Order the values power_db[u][j], j in E, by the unsigned key of
 * their bits, key = (bits & 0x80000000) ? ~bits : bits | 0x80000000 -- the usual float order, with -inf lowest and -0.0 below
 * +0.0; where a NaN falls is whatever the key gives and is not otherwise specified.  Then
 *   r = (uint64)floor_permille * (M - 1) / 1000 in integer arithmetic, floor_db[u] = the value of rank r (permille 0 asks for the
 *   default, 500: the median; 1000 is the maximum, SCN_FLOOR_MIN the minimum, rank 0; 1 ... 1000 are taken as they are, anything
 *   else is SCN_E_INVALID),
 *   cut[u] = floor_db[u] + threshold: ONE float addition -- in this mode `threshold` is an offset in the plan's own dB scale
 *   (10*log10|X|: 10 units are 20 dB of power) --, and bin j in E is a hit iff power_db[u][j] > cut[u], strictly as everywhere
 *   else.  A floor of -inf gives a cut of -inf, and bins at -inf are not hits.
 * An order statistic involves no float sum, so the floor, the cut and the hit list are exact: the same bits on every run and on
 * every route.  Records, their power_db, freq_hz, seq_id, their order and trigger (count > trigger_count) are those of a
 * fixed-threshold plan with that cut.  Frequency-domain plans with SCN_OUT_HITS only (SCN_E_INVALID at create otherwise); every
 * size scn_size_path supports, and averaged plans.  The transform runs as the spectrum-only plan's does and one detect kernel
 * follows it on the spectrum it stored (a hits-only plan keeps that spectrum in a buffer of its own); scn_collect_more,
 * scn_hits_view, scn_collect_signals and the gathers work as on any plan.  scn_collect_floor returns floor_db. */
enum {
  SCN_DETECT_FIXED = 0, /* power_db > threshold, one level for every unit */
  SCN_DETECT_FLOOR = 1, /* power_db > floor_db[unit] + threshold */
  SCN_DETECT_BASELINE = 2 /* power_db > baseline_db[row of the unit][bin] + threshold (below) */
};
#define SCN_FLOOR_MIN 0xffffffffu /* floor_permille: rank 0, the minimum (0 itself asks for the default, as SCN_DC_IGNORE_NONE) */

/* Floor window (scn_plan_set_floor_window): each bin's floor comes from its own neighbourhood -- order-statistic CFAR.  A floor
 * plan has a floor window (train, guard), initially none; without one the floor is the unit-wide one above.  With a window, for a
 * unit u and an evaluated bin with fftshift index i (natural bin j = (i + n/2) % n; the mask is the one above, as everywhere):
 *   reference cells of i: the EVALUATED bins at fftshift indices i' with guard < |i' - i| <= guard + train and 0 <= i' < n.
 *     Distances are in fftshift (frequency) order; there is no wrap between i = 0 and i = n - 1, which are opposite band edges.
 *     Bins the mask removes (outside [i_lo, i_hi], or in the DC window) take up distance but are not cells.  M_i is the number
 *     of cells: 2*train for interior bins, fewer near a band edge or the DC hole.
 *   r_i = (uint64)permille * (M_i - 1) / 1000 in integer arithmetic, permille from floor_permille exactly as above (0 -> 500,
 *     SCN_FLOOR_MIN -> 0); floor_i = the value of rank r_i among the cells in the key order above;
 *   cut_i = floor_i + threshold, ONE float addition; bin i is a hit iff power_db[u][j] > cut_i, strictly.
 * Records, their power_db, freq_hz, seq_id, their order and trigger are those of a plan that cut bin i at cut_i.  A NaN cell counts
 * as below nothing, whatever its sign: bin i is a hit iff at least r_i + 1 of its cells c have fl(c + threshold) < power_db[u][j],
 * which is the rank wording above for every window without a NaN cell -- and differs from it for a NaN whose sign bit is set, which
 * the key alone would place under every value.  (No transform of this library stores a unit that mixes NaN with other values: a NaN
 * sample makes the whole unit NaN, and such a unit has no hits.  scn_local_floor_from_spectrum, a host form of the ranks, places a
 * NaN as the key does.)  A unit that is all -inf has no hits.  No float sum is involved: the hit list is exact, the same bits on
 * every run and every route, as the unit-wide floor's.
 * Limits: 1 <= train <= SCN_FLOOR_TRAIN_MAX, guard <= SCN_FLOOR_GUARD_MAX.  A window under which some evaluated bin has M_i = 0
 * is SCN_E_INVALID: n = 16 with the default mask evaluates i in {2, 3, 4, 12, 13, 14}; (train 1, guard 0) is valid, (1, 1) is not
 * (bin 3's only candidates are i = 1, out of band, and i = 5, in the DC window).  That is a property of (n, mask, train, guard)
 * alone.  A windowed submit has no per-unit floor: scn_collect_floor on its slot is SCN_E_INVALID; scn_local_floor_from_spectrum
 * on the returned spectrum gives the per-bin floors. */
#define SCN_FLOOR_TRAIN_MAX 128u
#define SCN_FLOOR_GUARD_MAX 64u

/* Baseline detector (detect = SCN_DETECT_BASELINE): hits are what exceeds a stored spectrum -- what is here now that was not here
 * before.  A baseline plan owns baseline_db[rows][n]: float32, natural bin order, device memory; it has none at first
 * (scn_plan_set_baseline).  A unit is a buffer (for an averaged plan: the group).
 *   Row of a unit: unit u of a submit reads row (first + u) % rows, first = the submit's first_index for the indexed submits and 0
 *     otherwise; on an averaged plan u counts groups, as the frequency table does.  An indexed submit needs rows == the table's
 *     count or rows == 1, anything else is SCN_E_STATE; so is any submit on a plan that has no baseline.  Both are refused before
 *     anything is queued.
 *   Decision: an evaluated bin j (the mask of process.cpp:46-52, as everywhere) of unit u is a hit iff
 *     power_db[u][j] > baseline_db[row][j] + threshold: ONE float addition and a strict compare; `threshold` is an offset in the
 *     plan's own dB scale, as in floor mode.  So a NaN entry never produces a hit, nor does a +inf entry -- a caller's way to switch
 *     one bin of one row off --, a -inf entry produces a hit for every bin above -inf, and a bin that is itself -inf is never a hit.
 * No float is summed and nothing is selected: the hit list is exact, the same bits on every run and on every route.  Records, their
 * power_db, freq_hz, seq_id, their order and trigger are those of a plan that cut bin j at that value.  Frequency-domain plans with
 * SCN_OUT_HITS only (SCN_E_INVALID at create otherwise, before a device is looked for) -- and the flag is SET: a baseline plan names
 * its outputs, flags without SCN_OUT_SPECTRUM and SCN_OUT_HITS (elsewhere: both) are SCN_E_INVALID; every size scn_size_path
 * supports, and averaged plans; floor_permille is ignored.  The transform runs as the spectrum-only plan's does and one detect kernel, which only
 * reads the baseline, follows it on the spectrum it stored (a hits-only plan keeps that spectrum in a buffer of its own);
 * scn_collect_more, scn_hits_view, scn_collect_signals and the gathers work as on any plan; scn_collect_floor and
 * scn_plan_set_floor_window are SCN_E_INVALID.  The baseline changes only through scn_plan_set_baseline and
 * scn_plan_update_baseline, both refused while a submit is pending. */
enum {
  SCN_BASELINE_SET = 0, /* the row becomes the unit's spectrum, byte for byte */
  SCN_BASELINE_MAX = 1  /* per bin the larger of the two in the floor detector's key order (max-hold): exact, whatever the order */
};

/* Hit history (scn_plan_set_history): M-of-N confirmation, the binary integration that goes with a constant-false-alarm-rate
 * threshold -- a record counts only if its bin was a hit in at least M of the last N visits of its table entry.  Every detector above
 * decides on one unit alone; the history is what the plan remembers from one visit of a table entry to the next, across submits.
 * A plan may own a hit history: history[rows][n] of uint32_t and visits[rows] of uint32_t, device memory; it has none at first.  The
 * history is indexed by the FFTSHIFT index i of scn_hit.i (not by the natural bin).  Bit 0 of a word is the row's most recent visit,
 * bit k the visit k visits before it.  Open to every frequency-domain plan with SCN_OUT_HITS -- every detector, every size
 * scn_size_path supports, averaged plans (the unit is the group); a time-domain plan or one without SCN_OUT_HITS: SCN_E_INVALID.
 *   Row of a unit: unit u of a submit has row (first + u) % rows, first = the submit's first_index for the indexed submits and 0
 *     otherwise -- the baseline's rule.
 *   Fold (scn_plan_update_history): for every unit u of the slot's last collected submit, r its row, and for EVERY i in [0, n):
 *     history[r][i] = (history[r][i] << 1) | hit(u, i), hit(u, i) = 1 exactly when the submit's hit list holds a record (u, i) --
 *     a bin the mask removes shifts in 0 --, and visits[r] grows by one, saturating at 0xffffffff.  Rows no unit maps to are
 *     untouched.  All of the submit's hits take part, however many max_hits keeps.
 *   Confirmed: for 1 <= m <= window <= 32, a record (u, i) of the slot's ordered hit list is confirmed exactly when
 *     popcount(history[row(u)][i] & (window == 32 ? 0xffffffff : (1u << window) - 1)) >= m.  The zeros from before a row's first
 *     visit count as misses.  The confirmed list (scn_collect_confirmed) is the subsequence of the slot's full ordered hit list that
 *     passes: the same records bit for bit (seq_id, i, the bits of power_db, freq_hz), in the same order; m = window = 1 returns the
 *     full list.
 * Integers and compares only: the history and the confirmed list are exact, the same bits on every run and on every route.  No
 * kernel of a submit reads or writes the history: it changes only through scn_plan_set_history and scn_plan_update_history, both
 * allowed while other slots are pending.  A plan on which scn_plan_set_history is never called allocates nothing for it. */

/* Sweep trace (scn_plan_set_trace): the picture of the sweep -- one power-versus-frequency line across the whole table, in absolute
 * hertz, at a resolution the caller chooses: a panorama, a peak-hold line, a waterfall row.  A plan may own a trace; it has none at
 * first.  Its geometry is (f0_hz: uint64, cell_hz: uint32 >= 1, cells: 1 ... SCN_TRACE_CELLS_MAX): cell c covers the frequencies
 * [f0_hz + c * cell_hz, f0_hz + (c + 1) * cell_hz).  Per cell it holds max_db, min_db (float32) and count (uint64), device memory; an
 * empty cell reads max_db = -inf, min_db = +inf, count = 0.
 *   Which plans: frequency-domain plans with SCN_OUT_HITS whose submits store a spectrum -- SCN_OUT_SPECTRUM is set, or detect is
 *     SCN_DETECT_FLOOR or SCN_DETECT_BASELINE (those keep the spectrum their detect kernel reads) --; every size scn_size_path supports,
 *     and averaged plans (the unit is the group).  Anything else is SCN_E_INVALID from scn_plan_set_trace: a time-domain plan, a plan
 *     without SCN_OUT_HITS, a fixed-threshold hits-only plan (no spectrum exists anywhere).  SCN_OUT_HITS is required because only such
 *     submits stage their centre frequencies where a later kernel can read them.
 *   Fold (scn_plan_update_trace): for every unit u of the slot's last collected submit and every bin the mask of process.cpp:46-52
 *     lets through (fftshift index i, natural bin j = (i + n / 2) % n):
 *       f = the freq_hz a hit record of (u, i) would carry, bit for bit: uint64(fc - double(sample_rate / 2) + double(uint32(i *
 *         bin_step))), bin_step = sample_rate / n truncated, the cast the reference's x86-64 build makes (a negative double becomes
 *         the two's complement of its magnitude), fc the unit's centre exactly as its records get it: its own center_freqs entry, or
 *         table entry (first_index + u) % count;
 *       f < f0_hz: the bin is skipped; otherwise c = (f - f0_hz) / cell_hz in uint64 integer arithmetic, and c >= cells is skipped
 *         too.  (A negative start frequency wraps to a huge f and is therefore skipped.)
 *       v = power_db[u][j], read from the spectrum that submit stored.  A NaN is skipped and nothing changes.  Every other value,
 *         +-inf included, is folded: count[c] += 1, max_db[c] becomes the larger of itself and v, min_db[c] the smaller -- larger and
 *         smaller in the floor detector's key order, where -0.0 is below +0.0; the stored bits are the winning value's bits.
 * Maximum, minimum and an integer sum commute, so the trace is exact: the same bits on every run, route, partition and fold order.
 * No kernel of a submit reads or writes the trace: it changes only through scn_plan_set_trace and scn_plan_update_trace, both
 * allowed while other slots are pending.  A plan on which scn_plan_set_trace is never called allocates nothing for it. */
#define SCN_TRACE_CELLS_MAX (1u << 22)

/* Trace emitters (scn_plan_trace_emitters, scn_trace_emitters): the scanner's end product -- the emitters in the band, in absolute
 * hertz, one record per run of loud cells of a line of the trace.  Where a signal (below) never spans two units, an emitter is cut by
 * nothing but the trace's own cells: one that straddles the seam between two table entries, is seen by overlapping centres or was
 * on in every sweep is ONE record.  For a cell c of a window [first_cell, first_cell + cells) of a trace:
 *   Value: line SCN_TRACE_LINE_MAX: v = max_db[c]; SCN_TRACE_LINE_MIN: v = min_db[c]; SCN_TRACE_LINE_SPREAD: v = max_db[c] -
 *     min_db[c], one IEEE float32 subtraction, round to nearest, a denormal result kept; inf - inf is a NaN.
 *   On: cell c is on exactly when count[c] != 0, v is not a NaN, and v > threshold_db as float32 compares them (strict, as every
 *     detector here; -0.0 and +0.0 are equal).  threshold_db = -inf turns every non-empty cell on whose v is neither -inf nor a
 *     NaN; +inf turns nothing on.  Cells outside the window are off.
 *   Runs: the signals' rule, on cells.  In increasing c, an on cell starts a new emitter when it is the window's first on cell or
 *     when its c exceeds the previous on cell's by more than max_gap + 1.  Any uint32 max_gap is legal; an empty cell bridges as
 *     any other off cell does.
 *   The list is ordered by first_cell.  As scn_signal, the record has no mean and no float sum: every field is a pure function of
 *   the window, built from integers and compares (and the spread's one subtraction), the same bits on every run. */
enum { SCN_TRACE_LINE_MAX = 0, SCN_TRACE_LINE_MIN = 1, SCN_TRACE_LINE_SPREAD = 2 };
typedef struct scn_emitter { /* 56 bytes */
  uint64_t start_hz;    /* f0_hz + first_cell * cell_hz, uint64 arithmetic: the lower edge of the first on cell */
  uint64_t stop_hz;     /* f0_hz + (last_cell + 1) * cell_hz: the exclusive upper edge of the last on cell */
  uint64_t peak_hz;     /* f0_hz + peak_cell * cell_hz */
  uint64_t count;       /* sum of count[c] over the emitter's ON cells */
  uint32_t first_cell, last_cell; /* absolute cell indices of the trace (not window-relative) */
  uint32_t peak_cell;   /* the on cell with the largest v in the trace's key order (-0.0 below +0.0); equal keys: the lowest cell */
  uint32_t n_cells;     /* on cells (<= last_cell - first_cell + 1; equal when max_gap = 0) */
  float peak_db;        /* v at peak_cell, bit for bit */
  float peak_other_db;  /* MAX: min_db[peak_cell]; MIN and SPREAD: max_db[peak_cell]; bit for bit */
} scn_emitter;

/* Level histogram (scn_plan_set_levels): how often each cell of a frequency grid was how loud -- what a channel's occupancy, a band's
 * amplitude distribution and a median (or any percentile) line across the whole table are read from, where the trace keeps only a
 * cell's two extremes.  A plan may own a level histogram; it has none at first.  It is independent of the plan's trace: a plan may
 * have both, on different grids.
 *   Geometry: the trace's cells (f0_hz: uint64, cell_hz: uint32 >= 1, cells: 1 ... SCN_TRACE_CELLS_MAX) and a level table
 *     edges_db[n_edges] of float32, 1 <= n_edges <= SCN_LEVELS_EDGES_MAX, with cells * (n_edges + 1) <= SCN_LEVELS_WORDS_MAX.
 *   Edges: no edge is a NaN, and the edges are strictly increasing in the floor detector's key order (the order max_db and min_db of
 *     the trace are held in): -inf and +inf are legal edges, and -0.0, +0.0 are two distinct edges in that order.  Anything else is
 *     SCN_E_INVALID, nothing changed.
 *   State: hist[cells][n_edges + 1] of uint64, device memory, the level index fastest; every counter starts at 0.
 *   Level of a value v that is not a NaN: level(v) = the number of edges e with key(e) <= key(v), 0 ... n_edges.  Level l holds
 *     edges_db[l - 1] <= v < edges_db[l] (level 0: everything below the first edge, level n_edges: everything from the last edge
 *     up); a value equal to an edge belongs to the level above it.
 *   Which plans: exactly those that can have a trace ("Sweep trace").
 *   Fold (scn_plan_update_levels): for every unit of the slot's last collected submit and every bin the mask lets through, the cell
 *     c is the trace's, step for step -- the same freq_hz, the same skips below f0_hz and at or beyond `cells`, the same centre --
 *     and v = power_db[u][j].  A NaN is skipped; every other value, +-inf included, does hist[c][level(v)] += 1.
 *   Summary (scn_plan_levels_summary, scn_levels_summary), per cell: total = the sum of hist[c][l] over all l; above = the sum over
 *     l >= level, for the caller's level in 0 ... n_edges; rank_level = the smallest l whose cumulative count hist[c][0] + ... +
 *     hist[c][l] exceeds r = floor(permille * (total - 1) / 1000), the caller's permille in 0 ... 1000 taken as it is (0 is the
 *     lowest occupied level, not a default; 500 the median's; 1000 the highest occupied level).  r is formed without an overflow:
 *     total - 1 = 1000 a + b, 0 <= b < 1000, r = permille * a + (permille * b) / 1000.  An empty cell reads rank_level =
 *     0xffffffff, above = 0, total = 0.
 * An integer sum commutes, so the histogram is exact: the same bits on every run, route, partition and fold order.  No kernel of a
 * submit reads or writes it: it changes only through scn_plan_set_levels and scn_plan_update_levels, both allowed while other slots
 * are pending.  A plan on which scn_plan_set_levels is never called allocates nothing for it. */
#define SCN_LEVELS_EDGES_MAX 255u
#define SCN_LEVELS_WORDS_MAX (1u << 24)

/* Signals (scn_collect_signals, scn_signals_from_hits): runs of nearby hits merged into one record each.  A plan's buffer is
 * its unit of output (for an averaged plan: the group).  The hits of one unit, in increasing i, are split into signals: a hit
 * starts a new signal when it is the unit's first hit or when its i exceeds the previous hit's i by more than max_gap + 1.
 * max_gap = 0 therefore merges strictly adjacent bins only; max_gap = g bridges up to g bins that are not hits, whether they lie
 * below the threshold or are masked out.  The DC mask removes 2*dc_ignore_bins - 1 bins around i = N/2 (7 at the default of 4),
 * so a signal straddling DC is reported as two unless max_gap >= 7.  A signal never spans two units.  The list is ordered by
 * (unit, first_i).  There is deliberately no summed or mean power: a float sum would depend on the order of summation, and
 * every field here is a pure function of the hit list, built from integers and float comparisons only. */
typedef struct scn_signal { /* 40 bytes */
  uint64_t seq_id;         /* of the buffer (the group's first buffer), as in scn_hit */
  uint64_t peak_freq_hz;   /* freq_hz of the peak hit, bit for bit what its scn_hit carries */
  uint32_t first_i, last_i; /* fftshift-ordered bins of the signal's first and last hit */
  uint32_t peak_i;         /* the hit with the largest power_db; equal powers: the lowest i */
  uint32_t n_hits;         /* hits in the signal (<= last_i - first_i + 1; equal when max_gap = 0) */
  float peak_power_db;     /* that hit's power_db, bit for bit */
  uint32_t bandwidth_hz;   /* (last_i - first_i + 1) * (sample_rate / n), uint32 arithmetic as process.cpp:39 */
} scn_signal;

#define SCN_DC_IGNORE_NONE 0xffffffffu
/* Submits a plan can have in flight (submit ... collect per slot).  Two cover kernel-only pipelines; with the ordered records
 * fetched every step a submit's chain is kernel + list + DMA + the caller's copy, and three or four in flight keep the GPU fed. */
#define SCN_NUM_SLOTS 4

typedef struct scn_plan scn_plan;

SCN_API const char *scn_error_name(int status);
/* Text of the most recent failure on this thread ("" if none). */
SCN_API const char *scn_last_error(void);
SCN_API uint32_t scn_abi_version(void);
/* Number of HIP devices visible to this process (0 and SCN_E_NO_DEVICE if none). */
SCN_API int scn_device_count(int *count);

/* Which implementation a frequency-domain plan of n points runs (needs no device): what a caller sizing its batches
 * wants to know, and what the parity tests walk so that no fused specialisation goes untested. */
enum {
  SCN_PATH_UNSUPPORTED = 0,
  SCN_PATH_FUSED = 1,     /* one launch, the FFT staged in LDS (the powers of two 16 ... 16384) */
  SCN_PATH_FOUR_STEP = 2, /* two launches around a work buffer (32768, 65536) */
  SCN_PATH_STAGED = 3,    /* never returned: kept so that the numbering stays (the staged radix passes are the transform
                             inside SCN_PATH_BLUESTEIN) */
  SCN_PATH_BLUESTEIN = 4  /* the staged path around a chirp-z convolution (sizes that are not powers of two) */
};
SCN_API int scn_size_path(uint32_t n, uint32_t *path);

SCN_API int scn_plan_create(const scn_plan_desc *desc, scn_plan **out);
/* Averaged plans: the number of workgroups (*parts) that share the K buffers of one group in a submit of n_buffers buffers
 * (1 for plain plans).  Chosen from the CU count, G and K: enough parts to fill the GPU when G is small, at least two buffers
 * per part, 1 when G alone fills it. */
SCN_API int scn_plan_average_parts(const scn_plan *plan, uint32_t n_buffers, uint32_t *parts);
SCN_API int scn_plan_destroy(scn_plan *plan);

/* Bytes of one raw buffer (N samples) in the plan's wire format. */
SCN_API int scn_buffer_bytes(const scn_plan *plan, size_t *bytes);

/* The plan's pinned host staging slot (max_batch raw buffers back to back),
 * slot in [0, SCN_NUM_SLOTS).  Replaces MemoryPool/SampleQueue storage
 * (memoryPool.h:32-77): producers write device-format IQ straight into it.
 * Plan-owned, valid until scn_plan_destroy; allocated on first use. */
SCN_API int scn_host_buffer(scn_plan *plan, int slot, void **ptr, size_t *bytes);

/* Asynchronously copy n_buffers raw buffers from the pinned slot to the GPU
 * and run convert -> window -> FFT -> dB -> threshold on the plan's stream.
 * center_freqs / seq_ids (n_buffers each, host) are the MessageHeader fields
 * m_frequency / m_sequenceId (messageQueue.h:25-26); seq_ids may be NULL
 * (0,1,2,...).  Returns without waiting for the GPU. */
SCN_API int scn_submit(scn_plan *plan, int slot, uint32_t n_buffers,
               const double *center_freqs, const uint64_t *seq_ids);

/* Same, for raw IQ already resident in device memory (d_raw: n_buffers raw
 * buffers back to back).  d_power_db: optional device destination for the
 * dB spectra (n_buffers*N floats); NULL uses the plan's own buffer. */
SCN_API int scn_submit_device(scn_plan *plan, int slot, const void *d_raw,
                      uint32_t n_buffers, const double *center_freqs,
                      const uint64_t *seq_ids, float *d_power_db);

/* The plan's frequency table, resident on the GPU: the reference builds its table once (frequencyTable.cpp:31-36) and the
 * source retunes through it in order, wrapping at the end (GetNextFrequency, frequencyTable.cpp:38-46), so the centre
 * frequencies of a launch's buffers are a run of consecutive entries.  scn_submit_indexed / scn_submit_device_indexed are
 * scn_submit / scn_submit_device for such a launch: buffer b carries center_freqs[(first_index + b) % count], and no
 * per-buffer header crosses the boundary (with seq_ids == NULL none at all: 16 bytes per buffer that made launches of
 * 16 ... 128-point buffers host-bound).  The records are the same, bit for bit.  count == 0 drops the table.  Not while a
 * submit is pending (SCN_E_STATE); lists of earlier submits can no longer be re-read afterwards (scn_collect_more). */
SCN_API int scn_plan_set_table(scn_plan *plan, const double *center_freqs, uint32_t count);
SCN_API int scn_submit_indexed(scn_plan *plan, int slot, uint32_t n_buffers, uint32_t first_index, const uint64_t *seq_ids);
SCN_API int scn_submit_device_indexed(scn_plan *plan, int slot, const void *d_raw, uint32_t n_buffers, uint32_t first_index,
                              const uint64_t *seq_ids, float *d_power_db);

/* Wait for the slot's submit and fetch results.  power_db: host, n_buffers*N
 * floats in natural FFT bin order (bin 0 = DC), or NULL.  hits: host array of
 * hit_cap entries or NULL; on return *n_hits is the total number of hits,
 * the list is ordered by (buffer order, i) as a single-threaded reference run
 * prints them (process.cpp:46-61) -- the ordering and the completion of the
 * records (seq_id, freq_hz) happen on the GPU, the call copies min(*n_hits,
 * hit_cap, max_hits) 24-byte records out of pinned memory and returns
 * SCN_E_TRUNCATED when that is not all of them.  trigger: n_buffers bytes,
 * process_fft's return value (hits > trigger_count) per buffer, or NULL.
 * With hits == NULL the call waits for the kernel and the per-buffer counts only. */
SCN_API int scn_collect(scn_plan *plan, int slot, float *power_db, scn_hit *hits,
                uint32_t hit_cap, uint32_t *n_hits, uint8_t *trigger);

/* Records [first, first + hit_cap) of the ordered hit list of the slot's last COLLECTED submit (valid until the
 * slot's next submit): how a caller with a bounded buffer walks a list of any length -- a wideband burst makes every
 * buffer of a batch report > 1047 hits (process.cpp:62) and the reference prints each of them.  *n_written receives
 * the number of records stored (0 once first >= n_hits). */
SCN_API int scn_collect_more(scn_plan *plan, int slot, uint32_t first, scn_hit *hits, uint32_t hit_cap, uint32_t *n_written);

/* Zero-copy alternative to the hits argument of scn_collect: the plan's own pinned copy of the ordered list
 * (min(n_hits, max_hits) records), valid from scn_collect until the slot's next submit. */
SCN_API int scn_hits_view(scn_plan *plan, int slot, const scn_hit **hits, uint32_t *n);

/* Signals of the slot's last COLLECTED submit (same validity as scn_collect_more: until the slot's next submit /
 * scn_plan_set_table).  Built on the GPU from ALL of the submit's hits, however many (not limited by max_hits).
 * Stores records [first, first + cap) of the ordered signal list; *n_signals = the total.  SCN_E_TRUNCATED when
 * first + cap < total (the records stored are valid), signals may be NULL with cap 0 to learn the total.
 * Frequency-domain plans with SCN_OUT_HITS only (SCN_E_INVALID otherwise); a pending slot, or one whose list is no
 * longer valid, is SCN_E_STATE.  Runs beside pending submits of other slots without disturbing them. */
SCN_API int scn_collect_signals(scn_plan *plan, int slot, uint32_t max_gap, uint32_t first,
                                scn_signal *signals, uint32_t cap, uint32_t *n_signals);

/* The same merge on a host hit list ordered as scn_collect returns it (for a gathered list on the root, and the
 * definition the GPU form is held to).  Needs no device.  A unit ends where seq_id changes or i does not increase.
 * n and sample_rate are the plan's (bandwidth_hz).  Stores the first min(total, cap) records, *n_signals = the total;
 * SCN_E_TRUNCATED when cap < total; signals may be NULL with cap 0. */
SCN_API int scn_signals_from_hits(const scn_hit *hits, uint64_t n_hits, uint32_t n, uint32_t sample_rate,
                                  uint32_t max_gap, scn_signal *signals, uint64_t cap, uint64_t *n_signals);

/* Floor-detector plans: floor_db[u] of every unit of the slot's last COLLECTED submit (one float per buffer; per group on an
 * averaged plan), valid as scn_collect_signals' input is: until the slot's next submit / scn_plan_set_table (SCN_E_STATE for a
 * pending slot or one never collected).  A plan that is not in floor mode: SCN_E_INVALID. */
SCN_API int scn_collect_floor(scn_plan *plan, int slot, float *floor_db);

/* The same definition on ONE unit's host spectrum (n floats, natural bin order), with the descriptor's zero defaults for
 * dc_ignore_bins, use_bandwidth and floor_permille: *floor_db = the value of that rank among the evaluated bins.  Needs no
 * device; the definition the GPU form is held to.  A mask that lets no bin through, or a permille outside the descriptor's
 * values, is SCN_E_INVALID. */
SCN_API int scn_floor_from_spectrum(const float *power_db, uint32_t n, uint32_t dc_ignore_bins, double use_bandwidth,
                                    uint32_t floor_permille, float *floor_db);

/* Floor plans only (SCN_E_INVALID otherwise).  From the next submit on, each bin's floor is the rank among its own reference cells
 * ("Floor window" above).  train_bins = 0 (with guard_bins = 0) returns to the unit-wide floor.  SCN_E_STATE while any slot is
 * pending; collected slots keep their lists.  Limits and the M_i >= 1 rule: SCN_E_INVALID, nothing changed. */
SCN_API int scn_plan_set_floor_window(scn_plan *plan, uint32_t train_bins, uint32_t guard_bins);

/* The same definition on ONE unit's host spectrum (n floats, natural bin order), with the descriptor's zero defaults for
 * dc_ignore_bins, use_bandwidth and floor_permille: floor_db[j] = floor_i for every evaluated bin, other entries left untouched
 * (train_bins = guard_bins = 0: the unit-wide floor in every evaluated entry).  Needs no device; the definition the GPU form is
 * held to.  Same rejections as scn_floor_from_spectrum, plus the window's. */
SCN_API int scn_local_floor_from_spectrum(const float *power_db, uint32_t n, uint32_t dc_ignore_bins, double use_bandwidth,
                                          uint32_t floor_permille, uint32_t train_bins, uint32_t guard_bins, float *floor_db);

/* Baseline plans only (SCN_E_INVALID otherwise).  Replaces the baseline with `rows` rows of n floats from host memory (natural bin
 * order).  baseline_db == NULL with rows > 0 makes `rows` rows of +inf: armed, but nothing can hit -- where learning starts.
 * rows == 0 drops the baseline.  SCN_E_STATE while any slot is pending.  Synchronous, like scn_plan_set_table, and waits for this
 * plan's streams only. */
SCN_API int scn_plan_set_baseline(scn_plan *plan, uint32_t rows, const float *baseline_db);

/* Folds the spectrum of the slot's last COLLECTED submit -- the one its detect kernel read, all n bins of every unit, not only the
 * evaluated ones -- into the rows of that submit's units, on the GPU: op = SCN_BASELINE_SET or SCN_BASELINE_MAX.  Needs units <=
 * rows, so that no row is written twice in one call (SCN_E_INVALID otherwise, as an unknown op), no pending slot on the plan, and
 * a slot submitted and collected since the plan was made (SCN_E_STATE otherwise).  Returns when the update is complete.  A submit
 * that wrote its spectrum into the caller's d_power_db is read from there: the caller keeps that memory intact until this call
 * has returned. */
SCN_API int scn_plan_update_baseline(scn_plan *plan, int slot, uint32_t op);

/* Copies rows [first_row, first_row + rows) of the baseline to out (host, rows * n floats): what a caller stores to keep a learnt
 * baseline across runs.  A range outside the baseline is SCN_E_INVALID. */
SCN_API int scn_plan_get_baseline(scn_plan *plan, uint32_t first_row, uint32_t rows, float *out);

/* Frequency-domain plans with SCN_OUT_HITS only (SCN_E_INVALID otherwise; so the four calls below).  Gives the plan a hit history of
 * `rows` rows ("Hit history" above), all words and visits zero; rows == 0 drops it (the allocation is kept for the next one).
 * Allowed at any time, pending slots or not: nothing asynchronous ever touches the history.  Every call starts a new epoch: slots
 * folded before it can no longer be confirmed. */
SCN_API int scn_plan_set_history(scn_plan *plan, uint32_t rows);

/* Folds the hits of the slot's last COLLECTED submit into the rows of its units, on the GPU, and returns when that is complete.
 * Refused before anything is queued: a pending slot, or one without a collected submit whose list is still on the device
 * (SCN_E_STATE); a plan without a history (SCN_E_STATE); more units than rows (SCN_E_INVALID: a row would be visited twice in one
 * call); an indexed submit with rows neither the table's count nor 1 (SCN_E_STATE); a submit that was already folded
 * (SCN_E_STATE).  OTHER slots may be pending: with several submits in flight a caller folds every sweep without draining its
 * pipeline.  A submit of zero units is SCN_OK and no visit. */
SCN_API int scn_plan_update_history(scn_plan *plan, int slot);

/* Copies rows [first_row, first_row + rows) of the history (rows * n words, by fftshift index) and of the visits (rows words) to
 * host memory; either pointer may be NULL.  A range outside the history is SCN_E_INVALID. */
SCN_API int scn_plan_get_history(scn_plan *plan, uint32_t first_row, uint32_t rows, uint32_t *history, uint32_t *visits);

/* The confirmed list of the slot's last collected submit: *n_confirmed = the number of its records confirmed at (m, window), records
 * [first, first + cap) of the confirmed list are stored; SCN_E_TRUNCATED when first + cap < *n_confirmed (the records stored are
 * valid), hits may be NULL with cap 0 to learn the total -- as scn_collect_signals.  m or window outside 1 <= m <= window <= 32:
 * SCN_E_INVALID.  The slot's submit must have been folded (scn_plan_update_history) and that fold must be the plan's LATEST -- no
 * other fold and no scn_plan_set_history since -- SCN_E_STATE otherwise; that is stricter than slots whose rows do not overlap would
 * need, and cannot be wrong.  May be called repeatedly with different (m, window); runs beside pending submits of other slots
 * without disturbing them. */
SCN_API int scn_collect_confirmed(scn_plan *plan, int slot, uint32_t m, uint32_t window, uint32_t first, scn_hit *hits, uint32_t cap,
                                  uint32_t *n_confirmed);

/* The same fold and the same confirmation on host memory (for a gathered list on the root, and the definition the GPU forms are held
 * to: the same bits).  Need no device.  history: rows * n words, visits: rows words; first as a submit's first_index (reduced modulo
 * rows).  hits is an ordered hit list as scn_collect returns it, walked unit by unit: unit u owns the maximal run of records at the
 * cursor whose seq_id equals unit_seq_ids[u] -- with unit_seq_ids == NULL the id is u, as a submit without ids gives it -- so the ids
 * of CONSECUTIVE units must differ (a unit without hits owns an empty run).  Records left over behind the last unit's run, or a
 * record with i >= n, are SCN_E_INVALID, and then nothing has been changed.  scn_history_fold_hits needs n_units <= rows
 * (SCN_E_INVALID).  scn_confirm_hits stores the first min(total, cap) confirmed records, *n_out = the total, SCN_E_TRUNCATED when
 * cap < total; out may be NULL with cap 0. */
SCN_API int scn_history_fold_hits(uint32_t *history, uint32_t *visits, uint32_t rows, uint32_t n, uint32_t first, uint32_t n_units,
                                  const uint64_t *unit_seq_ids, const scn_hit *hits, uint64_t n_hits);
SCN_API int scn_confirm_hits(const uint32_t *history, uint32_t rows, uint32_t n, uint32_t first, uint32_t n_units,
                             const uint64_t *unit_seq_ids, const scn_hit *hits, uint64_t n_hits, uint32_t m, uint32_t window,
                             scn_hit *out, uint64_t cap, uint64_t *n_out);

/* Gives the plan a sweep trace of `cells` cells of cell_hz hertz from f0_hz up ("Sweep trace" above), every cell empty; every call
 * resets every cell.  cells == 0 drops the trace (the allocation is kept for the next one).  Allowed at any time, pending slots or
 * not: nothing asynchronous ever touches the trace.  A plan that cannot have one (above), cell_hz == 0 with cells != 0, or cells >
 * SCN_TRACE_CELLS_MAX: SCN_E_INVALID, nothing changed. */
SCN_API int scn_plan_set_trace(scn_plan *plan, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells);

/* Folds the spectrum of the slot's last COLLECTED submit into the trace, on the GPU, and returns when that is complete.  Refused
 * before anything is queued: a pending slot, or one without a collected submit whose list is still on the device -- after the slot's
 * next submit or a scn_plan_set_table the centres are gone -- (SCN_E_STATE); a plan without a trace (SCN_E_STATE).  OTHER slots may
 * be pending.  A submit that wrote its spectrum into the caller's d_power_db is read from there: the caller keeps that memory intact
 * until this call has returned (the baseline's rule).  A submit of zero units is SCN_OK and folds nothing.  Folding the same slot
 * twice is allowed: it counts twice and leaves max_db and min_db as they are. */
SCN_API int scn_plan_update_trace(scn_plan *plan, int slot);

/* Copies cells [first_cell, first_cell + cells) of the trace to host memory; any of the three pointers may be NULL.  A range outside
 * the trace is SCN_E_INVALID. */
SCN_API int scn_plan_get_trace(scn_plan *plan, uint32_t first_cell, uint32_t cells, float *max_db, float *min_db, uint64_t *count);

/* The same fold on host memory: the definition the GPU form is held to (the same bits), and what a caller without the plan at hand
 * folds a collected spectrum with.  Needs no device.  max_db, min_db and count (`cells` entries each) are read and written:
 * scn_trace_init makes the empty trace, and calls accumulate.  power_db: n_units spectra of n floats, natural bin order;
 * center_freqs: one per unit; dc_ignore_bins and use_bandwidth with the descriptor's zero defaults.  A null array (power_db and
 * center_freqs: with n_units != 0), cell_hz == 0, cells outside 1 ... SCN_TRACE_CELLS_MAX, n == 0 or above 2^24, sample_rate == 0:
 * SCN_E_INVALID, nothing changed. */
SCN_API int scn_trace_fold_spectrum(float *max_db, float *min_db, uint64_t *count, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells,
                                    const float *power_db, uint32_t n_units, uint32_t n, uint32_t sample_rate, uint32_t dc_ignore_bins,
                                    double use_bandwidth, const double *center_freqs);
/* The empty trace: max_db = -inf, min_db = +inf, count = 0 in every cell (same limits on cells, no null array). */
SCN_API int scn_trace_init(float *max_db, float *min_db, uint64_t *count, uint32_t cells);
/* Cell by cell: count += src_count, max_db = the larger of the two, min_db = the smaller, in the same key order -- how the root of a
 * sharded sweep joins the ranks' traces of one geometry; merge(A, B) is the trace of everything folded into A or B. */
SCN_API int scn_trace_merge(float *max_db, float *min_db, uint64_t *count, const float *src_max, const float *src_min,
                            const uint64_t *src_count, uint32_t cells);

/* scn_trace_merge of a host window into cells [first_cell, first_cell + cells) of the plan's trace, on the GPU: count adds, max_db
 * and min_db hold in key order -- what the root of a sharded sweep takes each rank's trace in with before it asks for the band's
 * emitters, and how exact cell values are put into a plan's trace.  A plan that cannot have a trace: SCN_E_INVALID; one that has
 * none: SCN_E_STATE; a range outside the trace, a null array with cells != 0, or a NaN anywhere in src_max or src_min (the host
 * arrays are scanned before anything is uploaded: a plan's trace never holds a NaN): SCN_E_INVALID, nothing changed.  Afterwards the
 * trace is bit for bit what scn_trace_merge makes of the two.  Runs on the plan's side stream and returns synchronised: allowed
 * while slots are pending.  cells == 0 is SCN_OK. */
SCN_API int scn_plan_merge_trace(scn_plan *plan, uint32_t first_cell, uint32_t cells, const float *src_max, const float *src_min,
                                 const uint64_t *src_count);

/* The emitters ("Trace emitters" above) of cells [first_cell, first_cell + cells) of the plan's trace, built on the GPU: only the
 * records cross to the host.  *n_emitters = the total; records [first, first + cap) of the list are stored, SCN_E_TRUNCATED when
 * first + cap < total (the records stored are valid), out may be NULL with cap 0 to learn the total -- scn_collect_signals' paging.
 * Every call recomputes: pages agree as long as the trace does not change between the calls.  A plan that cannot have a trace, a
 * line above SCN_TRACE_LINE_SPREAD or a NaN threshold_db: SCN_E_INVALID; a plan without a trace: SCN_E_STATE; a range outside the
 * trace: SCN_E_INVALID.  cells == 0 is SCN_OK with no emitter.  Runs on the plan's side stream and returns synchronised, as
 * scn_plan_get_trace: allowed while slots are pending.  The record storage is the plan's, allocated at the first call and grown on
 * demand; a plan on which this is never called allocates nothing for it. */
SCN_API int scn_plan_trace_emitters(scn_plan *plan, uint32_t first_cell, uint32_t cells, uint32_t line, float threshold_db,
                                    uint32_t max_gap, uint32_t first, scn_emitter *out, uint32_t cap, uint32_t *n_emitters);

/* The same list from a window on host memory: the definition the GPU form is held to (the same bits), and what a caller with a
 * trace but no plan at hand uses.  Needs no device.  max_db, min_db and count are the window, `cells` entries each;
 * first_cell_index is the absolute index of their first cell (first_cell, last_cell, peak_cell and the hertz fields count from the
 * trace's cell 0).  Stores the first min(total, cap) records, *n_emitters = the total; SCN_E_TRUNCATED when cap < total; out may
 * be NULL with cap 0.  A null array, cell_hz == 0, cells outside 1 ... SCN_TRACE_CELLS_MAX, first_cell_index + cells above
 * SCN_TRACE_CELLS_MAX, a line above SCN_TRACE_LINE_SPREAD or a NaN threshold_db: SCN_E_INVALID. */
SCN_API int scn_trace_emitters(const float *max_db, const float *min_db, const uint64_t *count, uint64_t f0_hz, uint32_t cell_hz,
                               uint32_t cells, uint32_t first_cell_index, uint32_t line, float threshold_db, uint32_t max_gap,
                               scn_emitter *out, uint64_t cap, uint64_t *n_emitters);

/* Gives the plan a level histogram of `cells` cells of cell_hz hertz from f0_hz up and the n_edges + 1 levels of edges_db ("Level
 * histogram" above), every counter 0; every call zeroes the histogram.  cells == 0 drops it (the allocation is kept for the next
 * one; the other arguments are not looked at).  Allowed at any time, pending slots or not.  A plan that cannot have a trace, a
 * geometry outside the limits, a null, unordered or NaN-holding table: SCN_E_INVALID, nothing changed.  A failure of the device
 * (an allocation, a copy) leaves the plan without a histogram. */
SCN_API int scn_plan_set_levels(scn_plan *plan, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells, const float *edges_db, uint32_t n_edges);

/* Folds the spectrum of the slot's last COLLECTED submit into the histogram, on the GPU, and returns when that is complete.  The
 * call rules, the refusals and their order are scn_plan_update_trace's, with "no level histogram" (SCN_E_STATE) in the place of "no
 * trace".  Folding the same slot twice counts twice. */
SCN_API int scn_plan_update_levels(scn_plan *plan, int slot);

/* Copies cells [first_cell, first_cell + cells) of the histogram, (n_edges + 1) counters each, to host memory.  A range outside the
 * histogram is SCN_E_INVALID; hist may be NULL where cells is 0. */
SCN_API int scn_plan_get_levels(scn_plan *plan, uint32_t first_cell, uint32_t cells, uint64_t *hist);

/* The summary of cells [first_cell, first_cell + cells), reduced on the GPU: what a caller reads instead of the whole table.  Any
 * of the three outputs (`cells` entries each) may be NULL.  A range outside the histogram, permille > 1000 or level > n_edges:
 * SCN_E_INVALID. */
SCN_API int scn_plan_levels_summary(scn_plan *plan, uint32_t first_cell, uint32_t cells, uint32_t permille, uint32_t level,
                                    uint32_t *rank_level, uint64_t *above, uint64_t *total);

/* The same fold on host memory: the definition the GPU form is held to (the same bits).  Needs no device.  hist (cells * (n_edges +
 * 1) counters) is read and written: calls accumulate on what the caller zeroed.  The other arguments and their rules are
 * scn_trace_fold_spectrum's; a geometry or a table scn_plan_set_levels would refuse: SCN_E_INVALID, nothing changed. */
SCN_API int scn_levels_fold_spectrum(uint64_t *hist, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells, const float *edges_db, uint32_t n_edges,
                                     const float *power_db, uint32_t n_units, uint32_t n, uint32_t sample_rate, uint32_t dc_ignore_bins,
                                     double use_bandwidth, const double *center_freqs);
/* Counter by counter hist += src (cells * n_levels each, n_levels = n_edges + 1) -- how the root of a sharded sweep joins the ranks'
 * histograms of one geometry; merge(A, B) is the histogram of everything folded into A or B. */
SCN_API int scn_levels_merge(uint64_t *hist, const uint64_t *src, uint32_t cells, uint32_t n_levels);
/* The summary ("Level histogram" above) of every cell of a histogram on host memory; any of the three outputs may be NULL.
 * permille > 1000, level >= n_levels, a null hist or a size outside the limits: SCN_E_INVALID, nothing written. */
SCN_API int scn_levels_summary(const uint64_t *hist, uint32_t cells, uint32_t n_levels, uint32_t permille, uint32_t level,
                               uint32_t *rank_level, uint64_t *above, uint64_t *total);

/* Time-domain plans (mode = SCN_MODE_TIME_DOMAIN; ProcessSamples::DoTimeDomainThresholding,
 * process.cpp:203-237): wait for the slot's submit and fetch, per buffer, the maximum and
 * minimum of 10*log10|x| over its samples and above[b] = (max >= threshold), i.e. the
 * function's return value.  The reference's line
 *   "Max signal %f above threshold %f frequency %.0f, min %f"
 * is printed from max_db[b], the plan threshold, the buffer's centre frequency and min_db[b].
 * Any of the three outputs may be NULL. */
SCN_API int scn_collect_time_domain(scn_plan *plan, int slot, float *max_db, float *min_db,
                            uint8_t *above);

/* K1 alone, synchronously: convert n_buffers raw buffers (host memory, the plan's wire format) to
 * complex float exactly as the plan's kernels do (utility.cpp:9-84 with the plan's enob /
 * correct_dc), writing n_buffers*N {re,im} float pairs to out (host).  This is what the
 * triggered-capture writer needs (messageQueue.h:98-139 dumps fftwf_complex[N] records); it runs on
 * its own stream and does not disturb pending slots. */
SCN_API int scn_convert_raw(scn_plan *plan, const void *raw, uint32_t n_buffers, float *out);

/* Wait for the slot's submit without copying anything back. */
SCN_API int scn_wait(scn_plan *plan, int slot);

/* Plumbing for callers that keep results on the GPU or time the stream. */
SCN_API int scn_plan_stream(scn_plan *plan, void **hip_stream);
/* The stream slot's kernels run on (the plan's one compute stream unless SCN_PLAN_OVERLAP_SLOTS). */
SCN_API int scn_slot_stream(scn_plan *plan, int slot, void **hip_stream);
SCN_API int scn_device_spectrum(scn_plan *plan, int slot, float **d_power_db);
/* Window coefficients the plan uses (host copy, n floats). */
SCN_API int scn_plan_window(const scn_plan *plan, float *w, uint32_t n);

/* frequencyTable.cpp:9-37: centre frequencies f1 + i*step*fs covering
 * [start, stop).  Writes min(count, cap) entries, returns count in *count.
 * shard / n_shards select the contiguous index range a rank owns
 * (n_shards = 1, shard = 0 for the whole table): *first is its first index. */
SCN_API int scn_frequency_table(uint32_t sample_rate, double start, double stop,
                        double use_bandwidth, double dc_ignore_width,
                        uint32_t shard, uint32_t n_shards, double *out,
                        uint32_t cap, uint32_t *count, uint32_t *first);

/* ------------------------------------------------------------------------------------
 * Multi-GPU sweep (scan.cpp:211-239 run once per GPU over a shard of the frequency table): one
 * process -- or one thread -- per GPU, each with its own plan on the index range scn_frequency_table gives it; no
 * data-path collective.  The only exchange is the sweep's final hit list to the root over RCCL / xGMI:
 * ncclAllGather of the per-rank counts, then one group of ncclSend / ncclRecv straight into the rank-major
 * (= globally ordered, the shards being contiguous) list on the root.
 *   scn_comm_unique_id   rank 0 creates the rendezvous id (ncclGetUniqueId) and hands its SCN_COMM_ID_BYTES to the
 *                        other ranks by any means (the launcher's store, a file, MPI ...)
 *   scn_comm_create      every rank, collectively (ncclCommInitRank) on its device
 *   scn_gather_hits      collective: local = this rank's ordered list (host memory); on the root `all` receives
 *                        min(*n_total, all_cap) records (SCN_E_TRUNCATED if fewer than all -- nothing is lost, the rest
 *                        is read with scn_gather_fetch), per_rank[world_size] the counts; both may be NULL elsewhere, and
 *                        `all` may be NULL on the root too (learn *n_total first, then fetch into an exact-size array:
 *                        the records are exchanged ONCE either way).  *n_total is set on every rank.  Every rank runs the
 *                        same sequence of collective steps whatever happens to it locally (scn_gather_protocol.h): a rank
 *                        that cannot take part -- a failed staging copy or allocation, a null list, a root out of range, a
 *                        failed device selection, a plan slot that was never collected, the root's failure to make room
 *                        for the list -- ANNOUNCES that in the exchange instead of returning before it: every rank then
 *                        returns an error, nothing is transferred, no rank is left waiting.  Not covered: a null
 *                        communicator (nothing to take part with) and a communicator RCCL itself reports broken.
 *   scn_gather_hits_device  the same with this rank's part taken from a collected slot of its plan -- the ordered list
 *                        the compaction kernel left in device memory (scn_hits.hip) -- instead of a host array: no
 *                        device->host->device round trip in front of the send.  The slot must have been collected
 *                        (scn_collect) and hold at most max_hits records.
 *   scn_gather_fetch     NOT collective, root only: records [first, first + cap) of the last gathered list, from the
 *                        root's device copy
 *   scn_gather_layout    host-only helper: offsets[r] = first index of rank r's records in the gathered list,
 *                        offsets[world_size] = total
 *   scn_gather_post / scn_gather_wait   the STEADY-STATE form, for a list per sweep (the table wraps every sweep,
 *                        frequencyTable.cpp:39-47, and a GPU's share of a sweep takes tens of microseconds): collective and
 *                        ASYNCHRONOUS.  Every rank's part is the collected slot's device list (as scn_gather_hits_device) and
 *                        travels in ONE fixed-size message -- a header and cap_per_rank records, the same on every rank -- so
 *                        no counts are exchanged first and nothing waits for the host: pack -> one group of ncclSend / ncclRecv
 *                        -> compaction into the root's pinned list, all on the communicator's stream, overlapping the next
 *                        sweep's kernels.  scn_gather_post returns a ticket at once (up to SCN_GATHER_TICKETS in flight; the
 *                        slot must not be submitted again before its ticket has been waited for); scn_gather_wait blocks until
 *                        that post has completed and, on the root, hands out the rank-major list IN PLACE (pinned memory, valid
 *                        until SCN_GATHER_TICKETS further posts), its length and the per-rank counts.  A rank whose list exceeds
 *                        cap_per_rank sends its first cap_per_rank records (SCN_E_TRUNCATED from its post and from the root's
 *                        wait, per_rank holding the true counts); a rank that cannot prepare its part still sends its message,
 *                        marked, and the ROOT's wait reports it (SCN_E_COMM) -- unlike the forms above the other ranks do not
 *                        learn of it: that is the price of having no round trip.  Every rank posts the same sequence of
 *                        (root, cap_per_rank).
 * RCCL is loaded on first use (dlopen), not at link time.
 * ------------------------------------------------------------------------------------ */
#define SCN_COMM_ID_BYTES 128
#define SCN_GATHER_TICKETS 4 /* scn_gather_post: posts in flight per communicator */
typedef struct scn_comm scn_comm;
SCN_API int scn_comm_unique_id(void *id);
SCN_API int scn_comm_create(const void *id, int rank, int world_size, int device_id, scn_comm **out);
SCN_API int scn_comm_destroy(scn_comm *comm);
SCN_API int scn_gather_hits(scn_comm *comm, const scn_hit *local, uint32_t n_local, uint32_t root, scn_hit *all,
                    uint64_t all_cap, uint64_t *n_total, uint32_t *per_rank);
SCN_API int scn_gather_hits_device(scn_comm *comm, scn_plan *plan, int slot, uint32_t root, scn_hit *all, uint64_t all_cap,
                           uint64_t *n_total, uint32_t *per_rank);
SCN_API int scn_gather_fetch(scn_comm *comm, uint64_t first, scn_hit *out, uint64_t cap, uint64_t *n_written);
SCN_API int scn_gather_layout(const uint32_t *per_rank, uint32_t world_size, uint64_t *offsets);
SCN_API int scn_gather_post(scn_comm *comm, scn_plan *plan, int slot, uint32_t root, uint32_t cap_per_rank, uint32_t *ticket);
SCN_API int scn_gather_wait(scn_comm *comm, uint32_t ticket, const scn_hit **list, uint64_t *n_total, uint32_t *per_rank);

/* HackRFSource::interpolateSamples (hackRFSource.cpp:186-222), the in-band header of HackRF
 * sweep-mode transfers: when the transfer starts with the bytes 0x7F 0x7F, bytes 2..9 hold the
 * tuned frequency in Hz (little-endian u64) and the first five int8 IQ samples (bytes 0..9) are
 * overwritten in place with the sixth (bytes 10,11).  *center_frequency receives
 * double(frequency + scan_offset_hz) (:221), i.e. double(scan_offset_hz) when no header is found.
 * Host-only (12 bytes of work per transfer; the frequency is needed on the host for scn_submit's
 * center_freqs anyway), needs no device.  Reproduces the reference as written: its loop over
 * 8192-sample blocks (:191-192) re-reads the START of the transfer every iteration, so only block
 * 0's header is ever parsed and later blocks are passed through untouched; a later iteration
 * matches again only when the patched sample is itself (0x7F,0x7F), in which case the frequency is
 * re-read from the patched bytes and the patch value is averaged with the sample before the block
 * (:210-213) -- also reproduced.  *n_mismatch (optional) counts the iterations at which the
 * reference prints "interpolateSamples: frequencyHz[..] != thisFrequencyHz[..]" (:204-208); the
 * library itself prints nothing. */
SCN_API int scn_hackrf_sweep_fixup(void *transfer, uint32_t valid_length, uint32_t scan_offset_hz,
                           double *center_frequency, uint32_t *n_mismatch);

/* ------------------------------------------------------------------------------------
 * Streaming Welch PSD (BASELINE config 5).  No counterpart in the reference -- it never
 * overlaps or averages -- so these entry points replace nothing; they
 * reuse its arithmetic: the converters of utility.cpp:9-84, the window of process.cpp:14-21,
 * the forward FFT of fft.cpp:20-25, the dB map of utility.cpp:86-98.  Definition: segments of
 * n samples every n/2 (50 % overlap), |X|^2 averaged over segments_per_psd consecutive
 * segments, output psd_db[k] = 5*log10(mean |X[k]|^2), natural bin order.  A submit of n_psd
 * PSDs consumes (n_psd*segments_per_psd + 1) * n/2 contiguous samples.
 * The mean is a float, defined as the PRODUCT  sum * (1.0f / (float)segments_per_psd)  of the float sum of the segments' float
 * powers (added in segment order within a row part, the parts in order) with the float reciprocal -- one float, whichever
 * kernel finishes the PSD (scn_welch_partition's *parts == 1 or > 1); the dB map of every plan is applied to that float.  A
 * division by segments_per_psd (the CPU oracle's form) gives the same float where segments_per_psd is a power of two and a
 * float at most one ulp away otherwise: about 2.6e-7 dB, under the map's own bound (tests/test_welch_exact_gpu.py).
 * Wire formats: the stream arrives as a device front-end delivers it (int8 HackRF
 * hackRFSource.cpp:261, int16 bladeRF bladerfSource.cpp:297, planar int16 SDRplay
 * sdrplaySource.cpp:197, float Airspy airspySource.cpp:197), in DELIVERY BLOCKS of n/2 samples
 * -- one SampleQueue::AppendSamples call each (messageQueue.h:190-237) -- back to back, and K1
 * is applied per block on the GPU: with correct_dc the integer mean removed is the block's
 * (utility.cpp:70-79 sums over the call's count), planar int16 is I[n/2] then Q[n/2] per
 * block.  Float samples are taken as they are (messageQueue.h:229-236).
 * Same slot / status conventions as scn_plan.  The pinned path (scn_welch_submit) replays a
 * captured hipGraph: H2D copy -> (block sums) -> column kernel -> row kernel -> D2H copy of the PSDs.
 * ------------------------------------------------------------------------------------ */
typedef struct scn_welch_desc {
  uint32_t struct_size;
  uint32_t n;                /* segment length; 65536 */
  uint32_t segments_per_psd; /* K >= 1 */
  uint32_t window_type;      /* 0 -> SCN_WIN_BLACKMAN_HARRIS */
  uint32_t max_psd;          /* PSDs per submit (>= 1) */
  int32_t device_id;
  uint32_t sample_kind;      /* SCN_KIND_*; 0 -> SCN_KIND_FLOAT_COMPLEX */
  uint32_t enob;             /* effective bits of the integer kinds (scan.cpp:138,183); 0 -> 12 (int16) / 8 (int8) */
  uint32_t correct_dc;       /* SampleQueue correctDCOffset, per delivery block; ignored for float samples */
  uint32_t reserved[1];
} scn_welch_desc;

typedef struct scn_welch scn_welch;

SCN_API int scn_welch_create(const scn_welch_desc *desc, scn_welch **out);
SCN_API int scn_welch_destroy(scn_welch *w);
/* complex samples one submit of n_psd PSDs consumes (times 2 / 4 / 8 bytes per sample of the plan's wire format) */
SCN_API int scn_welch_samples(const scn_welch *w, uint32_t n_psd, size_t *n_samples);
/* How a submit of n_psd PSDs is split over workgroups (what a caller sizing max_psd, and the parity tests, want to know):
 * *parts = workgroups sharing the K segments of one PSD's row tile (fixed at create; > 1 adds the combine kernel),
 * *column_groups / *segments_per_group = the column kernel's contiguous runs of segments (the last group ragged); each may be NULL. */
SCN_API int scn_welch_partition(const scn_welch *w, uint32_t n_psd, uint32_t *parts, uint32_t *column_groups, uint32_t *segments_per_group);
/* pinned input staging slot (max_psd PSDs worth of samples in the plan's wire format), plan-owned */
SCN_API int scn_welch_host_buffer(scn_welch *w, int slot, void **ptr, size_t *bytes);
SCN_API int scn_welch_submit(scn_welch *w, int slot, uint32_t n_psd);
/* samples (the plan's wire format) already in device memory; d_psd_db optional device destination (n_psd*n floats) */
SCN_API int scn_welch_submit_device(scn_welch *w, int slot, const void *d_samples, uint32_t n_psd,
                            float *d_psd_db);
/* wait and fetch the n_psd*n dB values (psd_db may be NULL to only wait) */
SCN_API int scn_welch_collect(scn_welch *w, int slot, float *psd_db);

#ifdef __cplusplus
}
#endif
#endif
