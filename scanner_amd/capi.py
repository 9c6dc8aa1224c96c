"""ctypes binding of include/scanner_hip.h (libscanner_hip.so).

This is the Python twin of the stub a C++ maintainer would write against the header
(INTEGRATION.md).  It fails loudly when the library is missing: the product has no CPU path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCN_LIB selects an experiment build (scripts/build_variants.py); the product library otherwise
LIB_PATH = os.environ.get("SCN_LIB") or os.path.join(_HERE, "libscanner_hip.so")

OK, E_INVALID, E_HIP, E_NOMEM, E_STATE, E_TRUNCATED, E_NO_DEVICE, E_COMM = range(8)
KIND_BYTE_COMPLEX, KIND_SHORT, KIND_SHORT_COMPLEX, KIND_FLOAT_COMPLEX = 1, 2, 3, 4
MODE_TIME_DOMAIN, MODE_FREQUENCY_DOMAIN = 1, 2
WIN_RECTANGULAR, WIN_BLACKMAN_HARRIS = 3, 5
WIN_HANN, WIN_BLACKMAN, WIN_KAISER, WIN_BARTLETT, WIN_FLATTOP, WIN_HAMMING = 1, 2, 4, 6, 7, 8   # (0, GNU Radio's WIN_HAMMING, is "the default" here)
OUT_SPECTRUM, OUT_HITS = 1, 2
PLAN_OVERLAP_SLOTS = 4  # each slot on its own compute stream (scanner_hip.h)
DC_IGNORE_NONE = 0xFFFFFFFF
NUM_SLOTS = 4
ABI_VERSION = 6
AVG_DWELL, AVG_SWEEPS = 0, 1  # scn_plan_desc.average_layout
DETECT_FIXED, DETECT_FLOOR, DETECT_BASELINE = 0, 1, 2  # scn_plan_desc.detect
BASELINE_SET, BASELINE_MAX = 0, 1  # scn_plan_update_baseline's op
FLOOR_MIN = 0xFFFFFFFF  # scn_plan_desc.floor_permille: rank 0 (0 itself asks for the default, the median)
FLOOR_TRAIN_MAX, FLOOR_GUARD_MAX = 128, 64  # the floor window's limits (scn_plan_set_floor_window)
TRACE_CELLS_MAX = 1 << 22  # the most cells a sweep trace has (scn_plan_set_trace)
TRACE_LINE_MAX, TRACE_LINE_MIN, TRACE_LINE_SPREAD = 0, 1, 2  # the line of a trace whose emitters are asked for (SCN_TRACE_LINE_*)
LEVELS_EDGES_MAX, LEVELS_WORDS_MAX = 255, 1 << 24  # a level histogram's most edges, and most counters (scn_plan_set_levels)
LEVELS_NO_RANK = 0xFFFFFFFF  # rank_level of an empty cell
PATH_UNSUPPORTED, PATH_FUSED, PATH_FOUR_STEP, PATH_STAGED, PATH_BLUESTEIN = range(5)
COMM_ID_BYTES = 128
GATHER_TICKETS = 4

BYTES_PER_SAMPLE = {KIND_BYTE_COMPLEX: 2, KIND_SHORT: 4, KIND_SHORT_COMPLEX: 4, KIND_FLOAT_COMPLEX: 8}

# struct scn_hit
HIT_DTYPE = np.dtype([("seq_id", "<u8"), ("i", "<u4"), ("power_db", "<f4"), ("freq_hz", "<u8")], align=True)
assert HIT_DTYPE.itemsize == 24
# struct scn_signal
SIGNAL_DTYPE = np.dtype([("seq_id", "<u8"), ("peak_freq_hz", "<u8"), ("first_i", "<u4"), ("last_i", "<u4"), ("peak_i", "<u4"),
                         ("n_hits", "<u4"), ("peak_power_db", "<f4"), ("bandwidth_hz", "<u4")], align=True)
assert SIGNAL_DTYPE.itemsize == 40


class Emitter(C.Structure):
    """struct scn_emitter"""
    _fields_ = [("start_hz", C.c_uint64), ("stop_hz", C.c_uint64), ("peak_hz", C.c_uint64), ("count", C.c_uint64), ("first_cell", C.c_uint32),
                ("last_cell", C.c_uint32), ("peak_cell", C.c_uint32), ("n_cells", C.c_uint32), ("peak_db", C.c_float), ("peak_other_db", C.c_float)]


EMITTER_DTYPE = np.dtype([("start_hz", "<u8"), ("stop_hz", "<u8"), ("peak_hz", "<u8"), ("count", "<u8"), ("first_cell", "<u4"), ("last_cell", "<u4"),
                          ("peak_cell", "<u4"), ("n_cells", "<u4"), ("peak_db", "<f4"), ("peak_other_db", "<f4")], align=True)
assert EMITTER_DTYPE.itemsize == 56 == C.sizeof(Emitter)


class PlanDesc(C.Structure):
    """struct scn_plan_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n", C.c_uint32),
        ("sample_rate", C.c_uint32),
        ("sample_kind", C.c_uint32),
        ("enob", C.c_uint32),
        ("correct_dc", C.c_uint32),
        ("window_type", C.c_uint32),
        ("mode", C.c_uint32),
        ("threshold", C.c_float),
        ("dc_ignore_bins", C.c_uint32),
        ("use_bandwidth", C.c_double),
        ("trigger_count", C.c_uint32),
        ("max_batch", C.c_uint32),
        ("max_hits", C.c_uint32),
        ("flags", C.c_uint32),
        ("device_id", C.c_int32),
        ("average", C.c_uint32),
        ("average_layout", C.c_uint32),
        ("detect", C.c_uint32),
        ("floor_permille", C.c_uint32),
        ("reserved", C.c_uint32 * 1),
    ]


class WelchDesc(C.Structure):
    """struct scn_welch_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n", C.c_uint32),
        ("segments_per_psd", C.c_uint32),
        ("window_type", C.c_uint32),
        ("max_psd", C.c_uint32),
        ("device_id", C.c_int32),
        ("sample_kind", C.c_uint32),
        ("enob", C.c_uint32),
        ("correct_dc", C.c_uint32),
        ("reserved", C.c_uint32 * 1),
    ]


# every symbol include/scanner_hip.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
SYMBOLS = {
    "scn_error_name": (C.c_char_p, [C.c_int]),
    "scn_last_error": (C.c_char_p, []),
    "scn_abi_version": (C.c_uint32, []),
    "scn_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "scn_size_path": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_plan_create": (C.c_int, [C.POINTER(PlanDesc), C.POINTER(_vp)]),
    "scn_plan_destroy": (C.c_int, [_vp]),
    "scn_plan_average_parts": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_buffer_bytes": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "scn_host_buffer": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "scn_submit": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, _vp]),
    "scn_submit_device": (C.c_int, [_vp, C.c_int, _vp, C.c_uint32, _vp, _vp, _vp]),
    "scn_plan_set_table": (C.c_int, [_vp, _vp, C.c_uint32]),
    "scn_submit_indexed": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, _vp]),
    "scn_submit_device_indexed": (C.c_int, [_vp, C.c_int, _vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "scn_collect": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint32), _vp]),
    "scn_collect_more": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_hits_view": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "scn_collect_signals": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_signals_from_hits": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "scn_collect_floor": (C.c_int, [_vp, C.c_int, _vp]),
    "scn_floor_from_spectrum": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_float)]),
    "scn_plan_set_floor_window": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "scn_local_floor_from_spectrum": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    "scn_plan_set_baseline": (C.c_int, [_vp, C.c_uint32, _vp]),
    "scn_plan_update_baseline": (C.c_int, [_vp, C.c_int, C.c_uint32]),
    "scn_plan_get_baseline": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "scn_plan_set_history": (C.c_int, [_vp, C.c_uint32]),
    "scn_plan_update_history": (C.c_int, [_vp, C.c_int]),
    "scn_plan_get_history": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "scn_collect_confirmed": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_history_fold_hits": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64]),
    "scn_confirm_hits": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                   _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "scn_plan_set_trace": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32]),
    "scn_plan_update_trace": (C.c_int, [_vp, C.c_int]),
    "scn_plan_get_trace": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "scn_trace_fold_spectrum": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_double, _vp]),
    "scn_trace_init": (C.c_int, [_vp, _vp, _vp, C.c_uint32]),
    "scn_trace_merge": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32]),
    "scn_plan_merge_trace": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "scn_plan_trace_emitters": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, _vp, C.c_uint32,
                                          C.POINTER(C.c_uint32)]),
    "scn_trace_emitters": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, _vp, C.c_uint64,
                                     C.POINTER(C.c_uint64)]),
    "scn_plan_set_levels": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32]),
    "scn_plan_update_levels": (C.c_int, [_vp, C.c_int]),
    "scn_plan_get_levels": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "scn_plan_levels_summary": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "scn_levels_fold_spectrum": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_double, _vp]),
    "scn_levels_merge": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32]),
    "scn_levels_summary": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "scn_collect_time_domain": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "scn_convert_raw": (C.c_int, [_vp, _vp, C.c_uint32, _vp]),
    "scn_wait": (C.c_int, [_vp, C.c_int]),
    "scn_plan_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "scn_slot_stream": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "scn_device_spectrum": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "scn_plan_window": (C.c_int, [_vp, _vp, C.c_uint32]),
    "scn_gather_post": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "scn_gather_wait": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), C.POINTER(C.c_uint64), _vp]),
    "scn_welch_create": (C.c_int, [C.POINTER(WelchDesc), C.POINTER(_vp)]),
    "scn_welch_destroy": (C.c_int, [_vp]),
    "scn_welch_samples": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_size_t)]),
    "scn_welch_partition": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "scn_welch_host_buffer": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "scn_welch_submit": (C.c_int, [_vp, C.c_int, C.c_uint32]),
    "scn_welch_submit_device": (C.c_int, [_vp, C.c_int, _vp, C.c_uint32, _vp]),
    "scn_welch_collect": (C.c_int, [_vp, C.c_int, _vp]),
    "scn_frequency_table": (C.c_int, [C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                      C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "scn_comm_unique_id": (C.c_int, [_vp]),
    "scn_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "scn_comm_destroy": (C.c_int, [_vp]),
    "scn_gather_hits": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "scn_gather_hits_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "scn_gather_fetch": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "scn_gather_layout": (C.c_int, [_vp, C.c_uint32, _vp]),
    "scn_hackrf_sweep_fixup": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double),
                                         C.POINTER(C.c_uint32)]),
}


class ScannerError(RuntimeError):
    def __init__(self, status, where, detail):
        self.status = status
        super().__init__(f"{where}: {detail} (status {status})")


_lib = None


def lib():
    """Load libscanner_hip.so (once).  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m scanner_amd.build` "
                "(hipcc --offload-arch=gfx950); scanner_amd has no CPU fallback")
        try:
            # share the process's HIP runtime with torch when torch is in use
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the pure C-ABI
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("SCN_LIB") and not hasattr(L, name):
                continue  # an experiment build (SCN_LIB) of an older tree may lack newer entry points; the product library may not
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.scn_abi_version() != ABI_VERSION:
            raise ImportError("libscanner_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(status, where):
    if status != OK:
        L = lib()
        raise ScannerError(status, where, f"{L.scn_error_name(status).decode()}: {L.scn_last_error().decode()}")


def size_path(n):
    """PATH_* of a frequency-domain plan of n points (scn_size_path; needs no device)."""
    out = C.c_uint32()
    check(lib().scn_size_path(int(n), C.byref(out)), "scn_size_path")
    return out.value


def frequency_table(sample_rate, start, stop, use_bandwidth=0.75, dc_ignore_width=0.0, shard=0, n_shards=1):
    """Centre frequencies of frequencyTable.cpp:9-37 (optionally one contiguous shard).
    Returns (first_index, float64 array)."""
    L = lib()
    cnt, first = C.c_uint32(), C.c_uint32()
    check(L.scn_frequency_table(int(sample_rate), start, stop, use_bandwidth, dc_ignore_width, shard, n_shards,
                                None, 0, C.byref(cnt), C.byref(first)), "scn_frequency_table")
    out = np.empty(cnt.value, np.float64)
    check(L.scn_frequency_table(int(sample_rate), start, stop, use_bandwidth, dc_ignore_width, shard, n_shards,
                                out.ctypes.data_as(_vp), cnt.value, C.byref(cnt), C.byref(first)),
          "scn_frequency_table")
    return first.value, out


def gather_layout(per_rank):
    """offsets[r] of rank r's records in the rank-major gathered hit list, total last (scn_gather_layout)."""
    per_rank = np.ascontiguousarray(per_rank, np.uint32)
    off = np.empty(per_rank.size + 1, np.uint64)
    check(lib().scn_gather_layout(per_rank.ctypes.data_as(_vp), per_rank.size, off.ctypes.data_as(_vp)), "scn_gather_layout")
    return off


def signals_from_hits(hits, n, sample_rate, max_gap=0):
    """scn_signals_from_hits: the hits of a list ordered as collect returns it (HIT_DTYPE), merged into signals (SIGNAL_DTYPE);
    n and sample_rate are the plan's.  Needs no device: the merge a root runs on a gathered list."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    L, total = lib(), C.c_uint64()
    st = L.scn_signals_from_hits(hits.ctypes.data_as(_vp), hits.size, int(n), int(sample_rate), int(max_gap), None, 0, C.byref(total))
    if st != E_TRUNCATED:
        check(st, "scn_signals_from_hits")
    out = np.zeros(total.value, SIGNAL_DTYPE)
    if total.value:
        check(L.scn_signals_from_hits(hits.ctypes.data_as(_vp), hits.size, int(n), int(sample_rate), int(max_gap),
                                      out.ctypes.data_as(_vp), out.size, C.byref(total)), "scn_signals_from_hits")
    return out


def _unit_ids(n_units, unit_seq_ids):
    if unit_seq_ids is None:
        return None, None
    ids = np.ascontiguousarray(unit_seq_ids, np.uint64)
    assert ids.size == n_units, f"{ids.size} unit ids for {n_units} units"
    return ids, ids.ctypes.data_as(_vp)


def history_fold_hits(history, visits, hits, n_units, first=0, unit_seq_ids=None):
    """scn_history_fold_hits: one submit's ordered hit list (HIT_DTYPE) folded IN PLACE into history (uint32 [rows, n], by fftshift
    index) and visits (uint32 [rows]) -- every word of the units' rows shifts left by one and takes the bin's hit bit.  Unit u has
    row (first + u) % rows and owns the run of records whose seq_id is unit_seq_ids[u] (None: u).  Needs no device."""
    assert history.dtype == np.uint32 and history.ndim == 2 and history.flags.c_contiguous and history.flags.writeable
    assert visits.dtype == np.uint32 and visits.shape == (history.shape[0],) and visits.flags.c_contiguous and visits.flags.writeable
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    ids, ids_ptr = _unit_ids(n_units, unit_seq_ids)
    check(lib().scn_history_fold_hits(history.ctypes.data_as(_vp), visits.ctypes.data_as(_vp), history.shape[0], history.shape[1], int(first),
                                      int(n_units), ids_ptr, hits.ctypes.data_as(_vp), hits.size), "scn_history_fold_hits")


def confirm_hits(history, hits, n_units, m, window, first=0, unit_seq_ids=None):
    """scn_confirm_hits: the records of an ordered hit list (HIT_DTYPE) whose history word has at least m of its `window` lowest bits
    set, in the list's order (HIT_DTYPE); history, first and unit_seq_ids as history_fold_hits takes them.  Needs no device."""
    history = np.ascontiguousarray(history, np.uint32)
    assert history.ndim == 2
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    ids, ids_ptr = _unit_ids(n_units, unit_seq_ids)
    out, total = np.zeros(hits.size, HIT_DTYPE), C.c_uint64()
    check(lib().scn_confirm_hits(history.ctypes.data_as(_vp), history.shape[0], history.shape[1], int(first), int(n_units), ids_ptr,
                                 hits.ctypes.data_as(_vp), hits.size, int(m), int(window), out.ctypes.data_as(_vp), out.size, C.byref(total)),
          "scn_confirm_hits")
    return out[: total.value]


def _trace_arrays(max_db, min_db, count):
    for a, dt in ((max_db, np.float32), (min_db, np.float32), (count, np.uint64)):
        assert a.dtype == dt and a.ndim == 1 and a.flags.c_contiguous and a.flags.writeable and a.size == max_db.size
    return max_db.ctypes.data_as(_vp), min_db.ctypes.data_as(_vp), count.ctypes.data_as(_vp)


def trace_init(cells):
    """scn_trace_init: the empty trace of `cells` cells -- (max_db float32 all -inf, min_db float32 all +inf, count uint64 all 0).
    Needs no device."""
    max_db, min_db, count = np.empty(cells, np.float32), np.empty(cells, np.float32), np.empty(cells, np.uint64)
    check(lib().scn_trace_init(*_trace_arrays(max_db, min_db, count), int(cells)), "scn_trace_init")
    return max_db, min_db, count


def trace_fold_spectrum(trace, f0_hz, cell_hz, power_db, sample_rate, center_freqs, dc_ignore_bins=4, use_bandwidth=0.75):
    """scn_trace_fold_spectrum: the spectra power_db (float32 [units, n], natural bin order) of units centred at center_freqs folded
    IN PLACE into trace = (max_db, min_db, count) on the grid (f0_hz, cell_hz, len(max_db)) -- what Plan.update_trace does on the
    GPU, to the bit (scanner_hip.h, "Sweep trace").  Needs no device."""
    max_db, min_db, count = trace
    power_db = np.ascontiguousarray(power_db, np.float32)
    assert power_db.ndim == 2
    fc = np.ascontiguousarray(center_freqs, np.float64).reshape(-1)
    assert fc.size == power_db.shape[0], f"{fc.size} centres for {power_db.shape[0]} units"
    check(lib().scn_trace_fold_spectrum(*_trace_arrays(max_db, min_db, count), int(f0_hz), int(cell_hz), max_db.size, power_db.ctypes.data_as(_vp),
                                        power_db.shape[0], power_db.shape[1], int(sample_rate),
                                        DC_IGNORE_NONE if dc_ignore_bins == 0 else int(dc_ignore_bins), float(use_bandwidth), fc.ctypes.data_as(_vp)),
          "scn_trace_fold_spectrum")


def trace_merge(trace, src):
    """scn_trace_merge: the trace src = (max_db, min_db, count) joined IN PLACE into trace, cell by cell -- the counts added, the
    larger maximum and the smaller minimum kept: how the root of a sharded sweep joins the ranks' traces.  Needs no device."""
    max_db, min_db, count = trace
    src_max, src_min, src_count = (np.ascontiguousarray(a, dt) for a, dt in zip(src, (np.float32, np.float32, np.uint64)))
    assert src_max.size == src_min.size == src_count.size == max_db.size
    check(lib().scn_trace_merge(*_trace_arrays(max_db, min_db, count), src_max.ctypes.data_as(_vp), src_min.ctypes.data_as(_vp),
                                src_count.ctypes.data_as(_vp), max_db.size), "scn_trace_merge")


def trace_emitters(trace, f0_hz, cell_hz, line, threshold_db, max_gap=0, first_cell=0):
    """scn_trace_emitters: the emitters (EMITTER_DTYPE, ordered by first_cell) of the window trace = (max_db, min_db, count) of a trace
    on the grid (f0_hz, cell_hz), whose first cell is cell first_cell of that trace -- one record per run of cells whose `line`
    (TRACE_LINE_*) is above threshold_db, runs joined across up to max_gap off cells: what Plan.trace_emitters builds on the GPU, to
    the bit (scanner_hip.h, "Trace emitters").  Needs no device."""
    max_db, min_db, count = (np.ascontiguousarray(a, dt) for a, dt in zip(trace, (np.float32, np.float32, np.uint64)))
    assert max_db.ndim == 1 and max_db.size == min_db.size == count.size
    L, total = lib(), C.c_uint64()
    args = (max_db.ctypes.data_as(_vp), min_db.ctypes.data_as(_vp), count.ctypes.data_as(_vp), int(f0_hz), int(cell_hz), max_db.size, int(first_cell),
            int(line), float(threshold_db), int(max_gap))
    st = L.scn_trace_emitters(*args, None, 0, C.byref(total))
    if st != E_TRUNCATED:
        check(st, "scn_trace_emitters")
    out = np.zeros(total.value, EMITTER_DTYPE)
    if total.value:
        check(L.scn_trace_emitters(*args, out.ctypes.data_as(_vp), out.size, C.byref(total)), "scn_trace_emitters")
    return out


def _levels_hist(hist):
    assert hist.dtype == np.uint64 and hist.ndim == 2 and hist.flags.c_contiguous and hist.flags.writeable
    return hist.ctypes.data_as(_vp)


def levels_fold_spectrum(hist, f0_hz, cell_hz, edges_db, power_db, sample_rate, center_freqs, dc_ignore_bins=4, use_bandwidth=0.75):
    """scn_levels_fold_spectrum: the spectra power_db (float32 [units, n], natural bin order) of units centred at center_freqs folded
    IN PLACE into hist (uint64 [cells, len(edges_db) + 1]) on the grid (f0_hz, cell_hz, cells) and the level table edges_db -- what
    Plan.update_levels does on the GPU, to the bit (scanner_hip.h, "Level histogram").  Needs no device."""
    edges = np.ascontiguousarray(edges_db, np.float32).reshape(-1)
    assert hist.shape[1] == edges.size + 1, f"{hist.shape[1]} levels for {edges.size} edges"
    power_db = np.ascontiguousarray(power_db, np.float32)
    assert power_db.ndim == 2
    fc = np.ascontiguousarray(center_freqs, np.float64).reshape(-1)
    assert fc.size == power_db.shape[0], f"{fc.size} centres for {power_db.shape[0]} units"
    check(lib().scn_levels_fold_spectrum(_levels_hist(hist), int(f0_hz), int(cell_hz), hist.shape[0], edges.ctypes.data_as(_vp), edges.size,
                                         power_db.ctypes.data_as(_vp), power_db.shape[0], power_db.shape[1], int(sample_rate),
                                         DC_IGNORE_NONE if dc_ignore_bins == 0 else int(dc_ignore_bins), float(use_bandwidth), fc.ctypes.data_as(_vp)),
          "scn_levels_fold_spectrum")


def levels_merge(hist, src):
    """scn_levels_merge: hist += src IN PLACE, counter by counter (uint64 [cells, n_levels] both) -- how the root of a sharded sweep
    joins the ranks' histograms.  Needs no device."""
    src = np.ascontiguousarray(src, np.uint64)
    assert src.shape == hist.shape
    check(lib().scn_levels_merge(_levels_hist(hist), src.ctypes.data_as(_vp), hist.shape[0], hist.shape[1]), "scn_levels_merge")


def levels_summary(hist, permille=500, level=0):
    """scn_levels_summary: per cell of hist (uint64 [cells, n_levels]) -> (rank_level uint32, above uint64, total uint64): the
    smallest level whose cumulative count exceeds floor(permille * (total - 1) / 1000) (0xFFFFFFFF in an empty cell), the counts of
    the levels >= level, and all counts.  Needs no device."""
    hist = np.ascontiguousarray(hist, np.uint64)
    assert hist.ndim == 2
    cells = hist.shape[0]
    rank, above, total = np.empty(cells, np.uint32), np.empty(cells, np.uint64), np.empty(cells, np.uint64)
    check(lib().scn_levels_summary(hist.ctypes.data_as(_vp), cells, hist.shape[1], int(permille), int(level), rank.ctypes.data_as(_vp),
                                   above.ctypes.data_as(_vp), total.ctypes.data_as(_vp)), "scn_levels_summary")
    return rank, above, total


def floor_from_spectrum(power_db, dc_ignore_bins=4, use_bandwidth=0.75, floor_permille=0):
    """scn_floor_from_spectrum: the floor detector's floor_db (np.float32) of ONE unit's dB spectrum (natural bin order) -- the value
    of rank floor_permille * (M - 1) // 1000 among the M evaluated bins (0: the median, FLOOR_MIN: the minimum).  Needs no device."""
    power_db = np.ascontiguousarray(power_db, np.float32).reshape(-1)
    out = C.c_float()
    check(lib().scn_floor_from_spectrum(power_db.ctypes.data_as(_vp), power_db.size, DC_IGNORE_NONE if dc_ignore_bins == 0 else int(dc_ignore_bins),
                                        float(use_bandwidth), int(floor_permille), C.byref(out)), "scn_floor_from_spectrum")
    return np.frombuffer(bytes(out), np.float32)[0]  # (the bits as they are: no detour through a Python float)


def local_floor_from_spectrum(power_db, train_bins, guard_bins=0, dc_ignore_bins=4, use_bandwidth=0.75, floor_permille=0, out=None):
    """scn_local_floor_from_spectrum: the floor window's per-bin floors of ONE unit's dB spectrum (natural bin order) -- float32 [n],
    entry j the value of rank floor_permille * (M_i - 1) // 1000 among the reference cells of the evaluated bin j (the evaluated bins
    guard_bins < |i' - i| <= guard_bins + train_bins away in fftshift order).  Entries of bins the mask removes are left as they are
    in `out` (NaN in a fresh array).  Needs no device."""
    power_db = np.ascontiguousarray(power_db, np.float32).reshape(-1)
    if out is None:
        out = np.full(power_db.size, np.nan, np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == power_db.size
    check(lib().scn_local_floor_from_spectrum(power_db.ctypes.data_as(_vp), power_db.size, DC_IGNORE_NONE if dc_ignore_bins == 0 else int(dc_ignore_bins),
                                              float(use_bandwidth), int(floor_permille), int(train_bins), int(guard_bins), out.ctypes.data_as(_vp)),
          "scn_local_floor_from_spectrum")
    return out


def hackrf_sweep_fixup(transfer, scan_offset_hz=0):
    """HackRFSource::interpolateSamples (hackRFSource.cpp:186-222) on a uint8/int8 numpy transfer,
    IN PLACE.  Returns (centre frequency, mismatch count)."""
    assert transfer.dtype.itemsize == 1 and transfer.flags.c_contiguous and transfer.flags.writeable
    fc, mism = C.c_double(), C.c_uint32()
    check(lib().scn_hackrf_sweep_fixup(transfer.ctypes.data_as(_vp), transfer.size, int(scan_offset_hz),
                                       C.byref(fc), C.byref(mism)), "scn_hackrf_sweep_fixup")
    return fc.value, mism.value
