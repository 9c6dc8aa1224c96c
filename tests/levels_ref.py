"""The level histogram as a numpy model, written from the definition in include/scanner_hip.h ("Level histogram") -- not from the
C code; the mask, a bin's frequency and the key are tests/trace_ref.py's, the trace's own model:

  a histogram is hist uint64 [cells, n_edges + 1], all 0 at first;
  for every unit u and every fftshift index i the mask lets through (natural bin j = (i + n // 2) % n):
    f as the trace's; f < f0 skipped; c = (f - f0) // cell_hz in uint64; c >= cells skipped;
    v = power_db[u][j]; NaN skipped; otherwise hist[c][level(v)] += 1, level(v) = the number of edges e with key(e) <= key(v);
  summary of a cell: total = sum of the row; above = sum of the levels >= level; rank_level = the smallest l whose cumulative count
    exceeds r = permille * (total - 1) // 1000 (Python integers: no overflow to think of); empty: (0xFFFFFFFF, 0, 0).

`mutant` names one deliberate error (tests/test_levels_cpu.py shows that the cases tell each of them from the definition)."""
import numpy as np

from tests import trace_ref

MUTANTS = ("edge_exclusive", "nan_counted", "mask_ignored", "levels_shifted", "index_exchanged")
NO_RANK = 0xFFFFFFFF


def new(cells, n_edges):
    return np.zeros((cells, n_edges + 1), np.uint64)


def edges_valid(edges_db):
    """no NaN, strictly increasing keys"""
    e = np.ascontiguousarray(edges_db, np.float32).reshape(-1)
    k = trace_ref.key(e).astype(np.int64)
    return 1 <= e.size <= 255 and not np.isnan(e).any() and bool(np.all(np.diff(k) > 0))


def level(edges_db, v, mutant=None):
    """int64 levels of float32 values v (no NaN among them, unless a mutant lets them through)"""
    ek = np.sort(trace_ref.key(np.ascontiguousarray(edges_db, np.float32).reshape(-1)).astype(np.int64))
    vk = trace_ref.key(v).astype(np.int64)
    lv = np.searchsorted(ek, vk, side="left" if mutant == "edge_exclusive" else "right")
    if mutant == "levels_shifted":
        lv = np.minimum(lv + 1, ek.size)
    return lv.astype(np.int64)


def fold(hist, f0_hz, cell_hz, edges_db, power_db, sample_rate, centres, dc_ignore_bins=4, use_bandwidth=0.75, mutant=None):
    """the histogram after the spectra power_db [units, n] (natural bin order) of units centred at `centres` were folded into it"""
    assert mutant is None or mutant in MUTANTS
    power_db = np.ascontiguousarray(power_db, np.float32)
    units, n = power_db.shape
    cells, n_levels = hist.shape
    assert n_levels == np.size(edges_db) + 1
    i = np.arange(n)
    j = (i + n // 2) % n
    ev = np.ones(n, bool) if mutant == "mask_ignored" else trace_ref.evaluated(n, dc_ignore_bins, use_bandwidth)
    out = hist.copy()
    flat = out.reshape(-1)
    for u in range(units):
        f = trace_ref.bin_freqs(n, sample_rate, centres[u])
        v = power_db[u][i if mutant == "index_exchanged" else j]
        ok = ev & (f >= np.uint64(f0_hz))
        if mutant != "nan_counted":
            ok &= ~np.isnan(v)
        c = (f[ok] - np.uint64(f0_hz)) // np.uint64(cell_hz)
        inside = c < np.uint64(cells)
        v = v[ok][inside]
        lv = np.minimum(level(edges_db, v, mutant), n_levels - 1)  # (a counted NaN: wherever its key falls)
        np.add.at(flat, c[inside].astype(np.int64) * n_levels + lv, np.uint64(1))
    return out


def summary(hist, permille, level_):
    """(rank_level uint32, above uint64, total uint64) per cell, in Python integers"""
    cells, n_levels = hist.shape
    assert 0 <= permille <= 1000 and 0 <= level_ < n_levels
    rank, above, total = np.empty(cells, np.uint32), np.empty(cells, np.uint64), np.empty(cells, np.uint64)
    for c in range(cells):
        row = [int(x) for x in hist[c]]
        t = sum(row)
        total[c], above[c] = t, sum(row[level_:])
        rank[c] = NO_RANK
        if t:
            r = permille * (t - 1) // 1000
            cum = 0
            for l, x in enumerate(row):
                cum += x
                if cum > r:
                    rank[c] = l
                    break
    return rank, above, total


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def describe(got, want):
    """where two histograms differ (for an assertion's message)"""
    if got.shape != want.shape:
        return f"shape {got.shape} for {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return "equal"
    return f"{len(bad)} counters differ, first (cell, level) {bad[:4].tolist()}: got {[int(got[tuple(b)]) for b in bad[:4]]}, want {[int(want[tuple(b)]) for b in bad[:4]]}"
