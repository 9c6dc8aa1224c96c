"""The floor window (scanner_hip.h, "Floor window") restated in numpy, vectorised: the keys of tests/floor_ref.py in fftshift order,
a sliding window over them, the cells the mask removes (and the slots beyond the band's edges: no wrap) mapped to the top key, a
row sort, and per row the rank from M_i -- the number of cells, counted on the mask and never on the values.  What
scn_local_floor_from_spectrum and the GPU's windowed detect kernel (scn_floor_local.hip) are held to, bit for bit.

NaN cells: the header's decision is the count of hit_bins_by_count -- a NaN cell counts as below nothing, whatever its sign --, which
the sort reproduces for every window without a NaN cell and for NaN cells whose sign bit is clear (their key is above +inf's).  A NaN
with its sign bit set has the lowest key: in a window that mixed such cells with finite ones the sort (and the host form, which ranks
by the key) would place it under every value, the count and the kernel above every value.  No transform stores such a unit -- a NaN
sample makes the whole unit NaN, which has no hits in either form -- so the two are held together on whole-NaN units only."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from scanner_amd import capi
from tests import floor_ref
from tests import tolerances as tol

TOP = np.uint32(0xFFFFFFFF)


def _geometry(n, train, guard, use_bandwidth=0.75, dc_ignore_bins=4):
    """(evaluated [n] by fftshift index i, natural bin j [n] of index i, the window's columns in a row of 2 (train + guard) + 1 slots)"""
    assert train >= 1 and guard >= 0
    i = np.arange(n)
    j = (i + n // 2) % n
    ev = tol.evaluated_mask(n, use_bandwidth, dc_ignore_bins)[j]
    reach = train + guard
    cols = np.concatenate([np.arange(-reach, -guard), np.arange(guard + 1, reach + 1)]) + reach
    return ev, j, cols


def _windows(by_i, fill, reach, rows, cols):
    """by_i [n] padded with `fill` beyond either end, then rows x cols of its sliding windows of 2 reach + 1 slots (a copy)"""
    padded = np.concatenate([np.full(reach, fill, by_i.dtype), by_i, np.full(reach, fill, by_i.dtype)])
    return sliding_window_view(padded, 2 * reach + 1)[np.ix_(rows, cols)]


def cell_counts(n, train, guard, use_bandwidth=0.75, dc_ignore_bins=4):
    """M_i of every evaluated bin, in increasing i"""
    ev, _, cols = _geometry(n, train, guard, use_bandwidth, dc_ignore_bins)
    return _windows(ev.astype(np.int32), 0, train + guard, np.flatnonzero(ev), cols).sum(axis=1)


def valid(n, train, guard, use_bandwidth=0.75, dc_ignore_bins=4):
    """the window's own rule: 1 <= train <= 128, guard <= 64, and every evaluated bin has a cell"""
    if not (1 <= train <= capi.FLOOR_TRAIN_MAX and 0 <= guard <= capi.FLOOR_GUARD_MAX):
        return False
    m = cell_counts(n, train, guard, use_bandwidth, dc_ignore_bins)
    return m.size > 0 and int(m.min()) >= 1


class WindowSort:
    """ONE unit's spectrum [n] under one window: the sorted cell keys of every evaluated bin (computed once; a rank per permille)"""

    def __init__(self, spectrum, train, guard, use_bandwidth=0.75, dc_ignore_bins=4):
        spectrum = np.ascontiguousarray(spectrum, np.float32).reshape(-1)
        self.n = n = spectrum.size
        ev, j, cols = _geometry(n, train, guard, use_bandwidth, dc_ignore_bins)
        self.i = np.flatnonzero(ev)  # the evaluated bins, in increasing i
        self.j = j[self.i]
        k = np.where(ev, floor_ref.keys(spectrum)[j], TOP)  # a bin that is not a cell sorts above every rank that is asked for
        self.cells = _windows(k, TOP, train + guard, self.i, cols)
        self.cells.sort(axis=1)
        self.m = _windows(ev.astype(np.int32), 0, train + guard, self.i, cols).sum(axis=1)
        assert self.m.size and self.m.min() >= 1, "the window leaves an evaluated bin without a cell"

    def ranks(self, floor_permille):
        return floor_ref.permille_of(floor_permille) * (self.m.astype(np.int64) - 1) // 1000

    def floors(self, floor_permille=0):
        """float32 [n] in natural bin order: floor_i of the evaluated bins, NaN elsewhere"""
        out = np.full(self.n, np.nan, np.float32)
        out[self.j] = floor_ref.unkeys(self.cells[np.arange(self.i.size), self.ranks(floor_permille)])
        return out


def floors(spectrum, train, guard, floor_permille=0, use_bandwidth=0.75, dc_ignore_bins=4):
    return WindowSort(spectrum, train, guard, use_bandwidth, dc_ignore_bins).floors(floor_permille)


def hit_bins(spectrum, floor_by_j, threshold, use_bandwidth=0.75, dc_ignore_bins=4):
    """the unit's hits in increasing i: (i, natural bin j) -- power_db[j] > floor_i + threshold, ONE float32 addition, strictly"""
    spectrum = np.ascontiguousarray(spectrum, np.float32)
    n = spectrum.size
    i = np.arange(n)
    j = (i + n // 2) % n
    ev = tol.evaluated_mask(n, use_bandwidth, dc_ignore_bins)[j]
    with np.errstate(invalid="ignore"):
        cut = floor_by_j[j] + np.float32(threshold)
        hit = ev & (spectrum[j] > cut)
    return i[hit], j[hit]


def hit_bins_by_count(spectrum, threshold, train, guard, floor_permille=0, use_bandwidth=0.75, dc_ignore_bins=4):
    """the same hits without a sort: bin i is a hit iff at least r_i + 1 of its cells c have fl(c + threshold) < power_db[j]"""
    spectrum = np.ascontiguousarray(spectrum, np.float32).reshape(-1)
    n = spectrum.size
    ev, j, cols = _geometry(n, train, guard, use_bandwidth, dc_ignore_bins)
    rows = np.flatnonzero(ev)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(ev, spectrum[j] + np.float32(threshold), np.float32(np.inf)).astype(np.float32)
        below = (_windows(w, np.float32(np.inf), train + guard, rows, cols) < spectrum[j][rows, None]).sum(axis=1)
    m = _windows(ev.astype(np.int32), 0, train + guard, rows, cols).sum(axis=1)
    need = floor_ref.permille_of(floor_permille) * (m.astype(np.int64) - 1) // 1000 + 1
    hit = below >= need
    return rows[hit], j[rows[hit]]


def detect(spectra, threshold, train, guard, floor_permille=0, center_freqs=None, seq_ids=None, fs=8000000, trigger_count=1047,
           use_bandwidth=0.75, dc_ignore_bins=4):
    """The whole windowed detector on the units' spectra [B, n]: (floors float32 [B, n] by natural bin, NaN where the mask removes the
    bin; records HIT_DTYPE ordered by (unit, i); trigger uint8 [B])"""
    spectra = np.ascontiguousarray(spectra, np.float32)
    nb, n = spectra.shape
    fc = np.zeros(nb) if center_freqs is None else np.asarray(center_freqs, np.float64)
    seq = np.arange(nb, dtype=np.uint64) if seq_ids is None else np.asarray(seq_ids, np.uint64)
    fl, recs, trig = np.empty((nb, n), np.float32), [], np.zeros(nb, np.uint8)
    for u in range(nb):
        fl[u] = floors(spectra[u], train, guard, floor_permille, use_bandwidth, dc_ignore_bins)
        ii, jj = hit_bins(spectra[u], fl[u], threshold, use_bandwidth, dc_ignore_bins)
        r = np.zeros(ii.size, capi.HIT_DTYPE)
        r["seq_id"], r["i"], r["power_db"] = seq[u], ii, spectra[u][jj]
        r["freq_hz"] = floor_ref._freq_hz(fc[u], ii, n, fs)
        recs.append(r)
        trig[u] = ii.size > trigger_count
    return fl, (np.concatenate(recs) if recs else np.zeros(0, capi.HIT_DTYPE)), trig
