"""The baseline detector (scanner_hip.h, "Baseline detector") restated in numpy: the row of a unit, the cut as one float32 addition
per bin, the hit set in increasing i over floor_ref's mask walk, and the two update operations on floor_ref's keys.  What the GPU's
detect and update kernels (scn_baseline.hip) are held to, bit for bit."""
import numpy as np

from scanner_amd import capi
from tests import tolerances as tol
from tests.floor_ref import _freq_hz, assert_same_records, hit_bins, keys, same_bits  # noqa: F401  (re-exported for the tests)


def rows_of(first, units, rows):
    """the baseline row of every unit of a submit: (first + u) % rows"""
    return (int(first) + np.arange(units)) % int(rows)


def cuts(baseline_row, threshold):
    """fl(baseline + threshold) per bin: ONE float32 addition"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.ascontiguousarray(baseline_row, np.float32) + np.float32(threshold)


def hits_of(spectrum, cut_by_bin, use_bandwidth=0.75, dc_ignore_bins=4):
    """one unit's hits in increasing i, (i, natural bin j), against a cut per natural bin.  floor_ref.hit_bins walks the mask: held
    against a cut of -inf it returns every evaluated bin above -inf, in increasing i -- and a bin at -inf (or NaN) is never a hit"""
    spectrum = np.ascontiguousarray(spectrum, np.float32)
    ii, jj = hit_bins(spectrum, -np.inf, use_bandwidth, dc_ignore_bins)
    with np.errstate(invalid="ignore"):
        hit = spectrum[jj] > cut_by_bin[jj]
    return ii[hit], jj[hit]


def detect(spectra, baseline, first, threshold, fc=None, seq=None, fs=8000000, trigger_count=1047, use_bandwidth=0.75, dc_ignore_bins=4):
    """The whole detector on the units' spectra [B, n] against baseline [rows, n]: (records HIT_DTYPE ordered by (unit, i), trigger
    uint8[B]).  fc / seq: per unit (zeros / the unit's index by default)."""
    spectra = np.ascontiguousarray(spectra, np.float32)
    baseline = np.ascontiguousarray(baseline, np.float32)
    nb, n = spectra.shape
    assert baseline.ndim == 2 and baseline.shape[1] == n
    fc = np.zeros(nb) if fc is None else np.asarray(fc, np.float64)
    seq = np.arange(nb, dtype=np.uint64) if seq is None else np.asarray(seq, np.uint64)
    row = rows_of(first, nb, baseline.shape[0])
    recs, trig = [], np.zeros(nb, np.uint8)
    for u in range(nb):
        ii, jj = hits_of(spectra[u], cuts(baseline[row[u]], threshold), use_bandwidth, dc_ignore_bins)
        r = np.zeros(ii.size, capi.HIT_DTYPE)
        r["seq_id"], r["i"], r["power_db"] = seq[u], ii, spectra[u][jj]
        r["freq_hz"] = _freq_hz(fc[u], ii, n, fs)
        recs.append(r)
        trig[u] = ii.size > trigger_count
    return (np.concatenate(recs) if recs else np.zeros(0, capi.HIT_DTYPE)), trig


def detect_brute(spectra, baseline, first, threshold, use_bandwidth=0.75, dc_ignore_bins=4):
    """the definition as a double loop over (unit, i), one scalar float32 at a time: [(unit, i, j)] -- what detect is checked against"""
    spectra = np.ascontiguousarray(spectra, np.float32)
    baseline = np.ascontiguousarray(baseline, np.float32)
    nb, n = spectra.shape
    rows = baseline.shape[0]
    half = n // 2
    use_window = int(use_bandwidth * n / 2.0)
    out = []
    for u in range(nb):
        r = (first + u) % rows
        for i in range(n):
            j = (i + half) % n
            if j < dc_ignore_bins or (n - j) < dc_ignore_bins or i < half - use_window or i > half + use_window:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                cut = np.float32(baseline[r, j]) + np.float32(threshold)
            if spectra[u, j] > cut:
                out.append((u, i, j))
    return out


def update(baseline, spectra, first, op):
    """scn_plan_update_baseline on a copy of baseline [rows, n]: every bin of row (first + u) % rows from unit u's spectrum --
    BASELINE_SET: its bits; BASELINE_MAX: the larger of the two in the key order (units <= rows)"""
    out = np.array(baseline, np.float32, copy=True)
    spectra = np.ascontiguousarray(spectra, np.float32)
    units = spectra.shape[0]
    assert units <= out.shape[0] and spectra.shape[1] == out.shape[1]
    for u, r in enumerate(rows_of(first, units, out.shape[0])):
        if op == capi.BASELINE_SET:
            out[r] = spectra[u]
        else:
            assert op == capi.BASELINE_MAX
            take = keys(spectra[u]) > keys(out[r])
            out[r].view(np.uint32)[take] = spectra[u].view(np.uint32)[take]
    return out


def evaluated(n):
    return tol.evaluated_mask(n)
