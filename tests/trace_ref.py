"""The sweep trace as a numpy model, written from the definition in include/scanner_hip.h ("Sweep trace") and from
process.cpp:36-57 -- not from the C code:

  a trace is (max_db float32 [cells], min_db float32 [cells], count uint64 [cells]); empty: (-inf, +inf, 0);
  for every unit u and every fftshift index i the mask lets through (natural bin j = (i + n // 2) % n):
    f = uint64(fc[u] - double(sample_rate // 2) + double(uint32(i * bin_step))), bin_step = sample_rate // n, a negative double
        becoming the two's complement of its magnitude;
    f < f0 skipped; c = (f - f0) // cell_hz in uint64; c >= cells skipped;
    v = power_db[u][j]; NaN skipped; otherwise count[c] += 1, max_db[c] / min_db[c] = the larger / smaller in the order of the key
        (bits & 0x80000000) ? ~bits : bits | 0x80000000, the winner's bits stored.

`mutant` names one deliberate error (tests/test_trace_cpu.py shows that the cases tell each of them from the definition)."""
import numpy as np

MUTANTS = ("untruncated_step", "mask_ignored", "nan_folded", "index_exchanged", "c_equal_cells_accepted")


def key(x):
    """the ordered key of float32 values: uint32, unsigned order = float order, -inf lowest, -0.0 below +0.0"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def new(cells):
    return np.full(cells, -np.inf, np.float32), np.full(cells, np.inf, np.float32), np.zeros(cells, np.uint64)


def same(a, b):
    """two traces are the same bits"""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and x.shape == y.shape
               for x, y in zip(a, b))


def describe(got, want):
    """where two traces differ (for an assertion's message)"""
    out = []
    for name, g, w in zip(("max_db", "min_db", "count"), got, want):
        bad = np.flatnonzero(np.ascontiguousarray(g).view(g.dtype.str.replace("f", "u")) != np.ascontiguousarray(w).view(w.dtype.str.replace("f", "u")))
        if bad.size:
            out.append(f"{name}: {bad.size} cells differ, first {bad[:4].tolist()}: got {g[bad[:4]].tolist()}, want {w[bad[:4]].tolist()}")
    return "; ".join(out) or "equal"


def evaluated(n, dc_ignore_bins=4, use_bandwidth=0.75):
    """bool [n] by fftshift index i: process.cpp:46-52 in uint32 arithmetic"""
    i = np.arange(n, dtype=np.int64)
    j = (i + n // 2) % n
    use_window = int(use_bandwidth * n / 2.0) & 0xFFFFFFFF
    lo, hi = (n // 2 - use_window) & 0xFFFFFFFF, (n // 2 + use_window) & 0xFFFFFFFF
    return ~((j < dc_ignore_bins) | ((n - j) < dc_ignore_bins)) & ~((i < lo) | (i > hi))


def bin_freqs(n, sample_rate, fc, mutant=None):
    """uint64 [n] by fftshift index: the freq_hz of a record of a unit centred at fc"""
    i = np.arange(n, dtype=np.uint64)
    start = np.float64(fc) - np.float64(sample_rate // 2)
    if mutant == "untruncated_step":
        offset = i.astype(np.float64) * (np.float64(sample_rate) / np.float64(n))
    else:
        offset = ((i * np.uint64(sample_rate // n)) & np.uint64(0xFFFFFFFF)).astype(np.float64)
    f = start + offset
    return np.trunc(f).astype(np.int64).astype(np.uint64)  # (|f| < 2^63: towards zero, then two's complement)


def _hold(trace, c, v):
    """values v (float32) into cells c (in range), any order: max / min by key, counts added"""
    max_db, min_db, count = trace
    kmax, kmin, k = key(max_db), key(min_db), key(v)
    np.maximum.at(kmax, c, k)
    np.minimum.at(kmin, c, k)
    cnt = count.copy()
    np.add.at(cnt, c, np.uint64(1))
    return unkey(kmax), unkey(kmin), cnt


def fold(trace, f0_hz, cell_hz, power_db, sample_rate, centres, dc_ignore_bins=4, use_bandwidth=0.75, mutant=None):
    """the trace after the spectra power_db [units, n] (natural bin order) of units centred at `centres` were folded into it"""
    assert mutant is None or mutant in MUTANTS
    power_db = np.ascontiguousarray(power_db, np.float32)
    units, n = power_db.shape
    cells = trace[0].size
    i = np.arange(n)
    j = (i + n // 2) % n
    ev = np.ones(n, bool) if mutant == "mask_ignored" else evaluated(n, dc_ignore_bins, use_bandwidth)
    cs, vs = [], []
    for u in range(units):
        f = bin_freqs(n, sample_rate, centres[u], mutant)
        v = power_db[u][i if mutant == "index_exchanged" else j]
        ok = ev & (f >= np.uint64(f0_hz))
        if mutant != "nan_folded":
            ok &= ~np.isnan(v)
        c = (f[ok] - np.uint64(f0_hz)) // np.uint64(cell_hz)
        v = v[ok]
        if mutant == "c_equal_cells_accepted":
            inside = c <= np.uint64(cells)
            c = np.minimum(c, np.uint64(cells - 1))
        else:
            inside = c < np.uint64(cells)
        cs.append(c[inside].astype(np.int64))
        vs.append(v[inside])
    if not cs:
        return tuple(a.copy() for a in trace)
    return _hold(trace, np.concatenate(cs), np.concatenate(vs))


def fold_hits(trace, f0_hz, cell_hz, hits):
    """the same from hit records (capi.HIT_DTYPE): each record's own freq_hz and power_db -- what the trace of a submit must be when
    every evaluated bin is a hit"""
    f = hits["freq_hz"].astype(np.uint64)
    ok = (f >= np.uint64(f0_hz)) & ~np.isnan(hits["power_db"])
    c = (f[ok] - np.uint64(f0_hz)) // np.uint64(cell_hz)
    inside = c < np.uint64(trace[0].size)
    return _hold(trace, c[inside].astype(np.int64), hits["power_db"][ok][inside].astype(np.float32))


def merge(a, b):
    return unkey(np.maximum(key(a[0]), key(b[0]))), unkey(np.minimum(key(a[1]), key(b[1]))), a[2] + b[2]
