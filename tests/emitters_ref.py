"""The trace emitters (include/scanner_hip.h, "Trace emitters") as a numpy model written from the definition: the value of a line, what
is on, the starts by the gap rule, the records.  Vectorised -- no Python loop over cells --, so a window of SCN_TRACE_CELLS_MAX cells
stays in seconds.  tests/test_emitters_cpu.py holds the host form (scn_trace_emitters) to it, tests/test_emitters_gpu.py the largest
window of the GPU form.

It also restates the launch shape of scanner_amd/csrc/scn_emitters.hip, as tests/trace_caps.py restates the fold's:

  kernel                        workgroups
  scn_emitters_count_kernel     ceil(tiles / 4): a TILE of 1024 cells per wave (16 trips of 64 cells), 4 waves per workgroup; no grid loop
  scn_emitters_build_kernel     the same
  scn_emitters_scan_kernel      1: 1024 threads, 4 consecutive tiles each (4096 tiles: the largest window's)

tests/test_emitters_cpu.py holds each number to the launcher's line."""
import numpy as np

from scanner_amd import capi

TILE = 1024           # `constexpr uint32_t kEmitTile = 1024;`
BLOCK = 256           # `constexpr uint32_t kEmitBlock = 256;`: a tile per wave
SCAN_BLOCK, SCAN_PER_THREAD = 1024, 4  # `constexpr uint32_t kEmitScanBlock = 1024, kEmitScanPerThread = 4;`

MUTANTS = ["ge", "gap", "empty_on", "peak_high", "count_span"]


def tiles(cells):
    return -(-cells // TILE)


def grid(cells):
    """workgroups of the count and build launches"""
    return -(-tiles(cells) // (BLOCK // 64))


def key(x):
    """the trace's ordered key of float32 values (unsigned order = float order, -0.0 below +0.0)"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def values(trace, line):
    """v per cell, float32"""
    max_db, min_db, _ = trace
    if line == capi.TRACE_LINE_MAX:
        return np.asarray(max_db, np.float32)
    if line == capi.TRACE_LINE_MIN:
        return np.asarray(min_db, np.float32)
    assert line == capi.TRACE_LINE_SPREAD
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(max_db, np.float32) - np.asarray(min_db, np.float32)  # (float32 - float32: one float32 subtraction, denormals kept)
    assert v.dtype == np.float32
    return v


def on_cells(trace, line, threshold_db, mutant=None):
    v, count = values(trace, line), np.asarray(trace[2], np.uint64)
    thr = np.float32(threshold_db)
    assert not np.isnan(thr)
    with np.errstate(invalid="ignore"):
        above = (v >= thr) if mutant == "ge" else (v > thr)
    on = (count != 0) & ~np.isnan(v) & above
    if mutant == "empty_on" and np.isneginf(thr):
        on |= count == 0
    return on


def emitters(trace, f0_hz, cell_hz, line, threshold_db, max_gap=0, first_cell=0, mutant=None):
    """the records (capi.EMITTER_DTYPE) of the window `trace`, whose first cell is cell first_cell of the whole trace"""
    max_db, min_db, count = (np.asarray(a, dt) for a, dt in zip(trace, (np.float32, np.float32, np.uint64)))
    v = values(trace, line)
    idx = np.flatnonzero(on_cells(trace, line, threshold_db, mutant)).astype(np.int64)
    out = np.zeros(0, capi.EMITTER_DTYPE)
    if idx.size == 0:
        return out
    bridge = int(max_gap) + (0 if mutant == "gap" else 1)
    start = np.concatenate([[True], np.diff(idx) > bridge])  # the window's first on cell, or more than max_gap + 1 beyond the previous
    at = np.flatnonzero(start)
    first, last = idx[start], idx[np.concatenate([start[1:], [True]])]
    out = np.zeros(at.size, capi.EMITTER_DTYPE)
    cell = (idx + int(first_cell)).astype(np.uint64)
    low = cell if mutant == "peak_high" else np.uint64(0xFFFFFFFF) - cell  # equal values: the lowest cell
    peak = np.maximum.reduceat((key(v[idx]).astype(np.uint64) << np.uint64(32)) | low, at)
    peak_low = peak & np.uint64(0xFFFFFFFF)
    peak_cell = (peak_low if mutant == "peak_high" else np.uint64(0xFFFFFFFF) - peak_low).astype(np.int64)
    w = peak_cell - int(first_cell)
    if mutant == "count_span":
        run = np.concatenate([[0], np.cumsum(count, dtype=np.uint64)]).astype(np.uint64)
        out["count"] = run[last + 1] - run[first]
    else:
        out["count"] = np.add.reduceat(count[idx], at)
    f0, hz = np.uint64(int(f0_hz) & 0xFFFFFFFFFFFFFFFF), np.uint64(cell_hz)
    with np.errstate(over="ignore"):  # uint64 arithmetic wraps, as the definition's
        out["start_hz"] = f0 + (first + int(first_cell)).astype(np.uint64) * hz
        out["stop_hz"] = f0 + (last + int(first_cell) + 1).astype(np.uint64) * hz
        out["peak_hz"] = f0 + peak_cell.astype(np.uint64) * hz
    out["first_cell"] = first + int(first_cell)
    out["last_cell"] = last + int(first_cell)
    out["peak_cell"] = peak_cell
    out["n_cells"] = np.diff(np.concatenate([at, [idx.size]]))
    out["peak_db"] = v[w]
    out["peak_other_db"] = (min_db if line == capi.TRACE_LINE_MAX else max_db)[w]
    return out


def same(a, b):
    """two record arrays, byte for byte"""
    return a.dtype == b.dtype == capi.EMITTER_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


def describe(got, want):
    if got.shape != want.shape:
        return f"{got.size} records, {want.size} wanted; first: got {got[:2]}, want {want[:2]}"
    bad = np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)][:100000])
    return f"{bad.size} records differ, the first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}" if bad.size else "equal"


def seeded_trace(cells, seed, p_empty=0.1):
    """a trace of dB-like values with max >= min, empty cells as the trace reads them (-inf, +inf, 0), counts 1 ... 9"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(cells) * 12.0 - 60.0).astype(np.float32)
    b = (a + np.abs(rng.standard_normal(cells) * 6.0).astype(np.float32)).astype(np.float32)
    count = rng.integers(1, 10, cells).astype(np.uint64)
    one = rng.random(cells) < 0.2  # a single value folded: max == min
    b[one] = a[one]
    count[one] = 1
    empty = rng.random(cells) < p_empty
    a[empty], b[empty], count[empty] = np.inf, -np.inf, 0
    return b, a, count
