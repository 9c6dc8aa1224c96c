"""The floor detector (scanner_hip.h, "Floor detector") restated in numpy: the key transform, the rank by np.sort of the keys over
tolerances.evaluated_mask, the cut as one float32 addition, the hit set in increasing i.  What scn_floor_from_spectrum and the
GPU's detect kernel (scn_floor.hip) are held to, bit for bit."""
import numpy as np

from scanner_amd import capi
from tests import tolerances as tol


def keys(power_db):
    """uint32 keys whose unsigned order is the float order of the values (-inf lowest, -0.0 below +0.0)"""
    bits = np.ascontiguousarray(power_db, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def permille_of(floor_permille):
    """the descriptor's field with its default applied: 0 -> 500, FLOOR_MIN -> 0"""
    if floor_permille == capi.FLOOR_MIN:
        return 0
    if floor_permille == 0:
        return 500
    assert 1 <= floor_permille <= 1000
    return int(floor_permille)


def floor_db(spectrum, floor_permille=0, use_bandwidth=0.75, dc_ignore_bins=4):
    """np.float32: the value of rank permille * (M - 1) // 1000 among the evaluated bins of ONE unit's spectrum [n]"""
    spectrum = np.ascontiguousarray(spectrum, np.float32)
    mask = tol.evaluated_mask(spectrum.size, use_bandwidth, dc_ignore_bins)
    k = np.sort(keys(spectrum[mask]))
    r = permille_of(floor_permille) * (k.size - 1) // 1000
    return unkeys(k[r:r + 1])[0]


def cut_of(floor, threshold):
    with np.errstate(invalid="ignore"):
        return np.float32(floor) + np.float32(threshold)


def hit_bins(spectrum, cut, use_bandwidth=0.75, dc_ignore_bins=4):
    """the unit's hits in increasing i: (i, natural bin j)"""
    spectrum = np.ascontiguousarray(spectrum, np.float32)
    n = spectrum.size
    mask = tol.evaluated_mask(n, use_bandwidth, dc_ignore_bins)
    i = np.arange(n)
    j = (i + n // 2) % n
    with np.errstate(invalid="ignore"):
        hit = mask[j] & (spectrum[j] > np.float32(cut))
    return i[hit], j[hit]


def _freq_hz(fc, i, n, fs):
    """process.cpp:38-39,55-57 for an array of bins i, with the x86-64 cast of a negative double (two's complement)"""
    i = np.asarray(i, np.uint64)
    f = (float(fc) - float(fs // 2)) + ((i * np.uint64(fs // n)) & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return np.trunc(f).astype(np.int64).view(np.uint64)


def detect(spectra, threshold, floor_permille=0, center_freqs=None, seq_ids=None, fs=8000000, trigger_count=1047,
           use_bandwidth=0.75, dc_ignore_bins=4):
    """The whole detector on the units' spectra [B, n]: (floors float32[B], records HIT_DTYPE ordered by (unit, i), trigger uint8[B])"""
    spectra = np.ascontiguousarray(spectra, np.float32)
    nb, n = spectra.shape
    fc = np.zeros(nb) if center_freqs is None else np.asarray(center_freqs, np.float64)
    seq = np.arange(nb, dtype=np.uint64) if seq_ids is None else np.asarray(seq_ids, np.uint64)
    floors, recs, trig = np.empty(nb, np.float32), [], np.zeros(nb, np.uint8)
    for u in range(nb):
        floors[u] = floor_db(spectra[u], floor_permille, use_bandwidth, dc_ignore_bins)
        ii, jj = hit_bins(spectra[u], cut_of(floors[u], threshold), use_bandwidth, dc_ignore_bins)
        r = np.zeros(ii.size, capi.HIT_DTYPE)
        r["seq_id"], r["i"], r["power_db"] = seq[u], ii, spectra[u][jj]
        r["freq_hz"] = _freq_hz(fc[u], ii, n, fs)
        recs.append(r)
        trig[u] = ii.size > trigger_count
    return floors, (np.concatenate(recs) if recs else np.zeros(0, capi.HIT_DTYPE)), trig


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same_records(got, want, what):
    """record for record: i, the bits of power_db, freq_hz, seq_id, and with them the order"""
    assert len(got) == len(want), f"{what}: {len(got)} records, expected {len(want)}"
    for f in ("seq_id", "i", "freq_hz"):
        assert np.array_equal(got[f], want[f]), f"{what}: {f} differs"
    assert same_bits(got["power_db"], want["power_db"]), f"{what}: power_db differs"
