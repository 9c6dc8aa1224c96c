"""The parity bar, written down once (BASELINE.json north_star: "power spectra within 1e-5
relative float tolerance, bin indices of detected peaks bit-exact").

float32 FFTs of different butterfly order differ by ~1e-7 of the buffer's RMS level in every
bin, so a bin far below the mean (a Rayleigh-small bin) has an unbounded *per-bin* relative
error even between two correct implementations (complex64 vs
complex128 FFT already shows per-bin max 1.9e-4).  "1e-5 relative" is therefore taken
relative to max(P_bin, mean P of the buffer) on linear power for EVERY bin, and on the dB
output as 1e-5*|dB| + 1e-4 for every bin at or above the buffer's mean power -- the bins a
threshold detector can report (a 1e-4 dB step is a 4.6e-5 relative power step; the ~1e-6
of the buffer's RMS level that two float32 FFTs differ by exceeds that on bins 20 dB down).
The strict per-bin figure is computed and reported by the tests too.

SAID PLAINLY, because a green suite could be misread otherwise: the 1e-5 of north_star is met in the sense "relative to
max(bin, buffer mean)".  The dB criterion is only ASSERTED on bins at or above the buffer's mean power; over ALL bins the
same runs show max dB errors of ~1.3e-3 dB and strict per-bin relative power errors of ~6e-4 (the keys
max_db_err_all_bins / strict_per_bin_rel_power_max of compare_spectra's result, printed by smoke()): that is the float32
noise floor on Rayleigh-small bins, present between any two float32 FFTs (the reference's FFTW included), not an
implementation error -- but it is not "1e-5 per bin" either.  And the oracle these figures are taken against is itself pinned
by float64 mathematics only, not by the reference's own output (parity unpinned).

THE THIRD CRITERION (floor_errors; tests/test_dynamic_range_cpu.py, tests/test_dynamic_range_gpu.py).  Under one strong signal nearly
every bin lies below 1e-5 of the buffer's mean power (88 % at 64 points, over 99 % from 4096 up): there the first criterion allows an
error of a hundred times the bin, and flip_unsafe takes the bin out of the hit comparison.  On exactly those bins floor_errors measures
|a_test - a_float64| in amplitude, less the dB map's own proven allowance, relative to the buffer's rms level, and a kernel must stay
within twice what the larger of two float32 transforms that are not the kernel gives on the same buffers (the oracle's chain and
scipy.fft on complex64: 3e-7 at 16 points, 3e-6 at 4096, 6e-6 ... 1.1e-5 at 65536 -- Y is a maximum over a launch's floor bins and
moves by up to 2x with the draw of the scene; profiles/dynamic_range.txt has the figure of every launch).  Hit lists on those scenes are demanded exact wherever the float64
amplitude is further than that bound from the threshold.  This closes the gap of four orders of magnitude in which a coarse twiddle
table or a float pass where double is promised would raise the floor by tens of dB unnoticed.  WHAT REMAINS UNASSERTED: a bin between
the floor criterion's limit (1e-5 of the mean) and the mean itself is still held to 1e-5 of the MEAN only, i.e. to 1e-5 ... 1 of its
own power; the criterion is asserted on the scenes of tests/dr_scenes.py, not on the suite's other inputs; and a SINGLE table entry
ten ulp off is seen only where it carries enough of a buffer's energy to rise over a float32 transform's own rounding -- at 16 ... 128
points, and in the table a workgroup shares up to 1024 points; from 4096 points up, and for one thread's pass-1 constant from 512 up,
it stays under Y and unseen (measured: the docstring of tests/test_dynamic_range_gpu.py).
"""
import numpy as np

REL_POWER = 1e-5
DB_REL = 1e-5
DB_ABS = 1e-4
DB_MIN_POWER_RATIO = 1.0     # dB criterion applies to bins with P >= this * mean(P)
GUARD_DB = 1e-3              # no evaluated bin may sit this close to the threshold

# The device's dB map (scn_device.h): the product form below SCN_P_EXACT_FROM = 10^3.2 (16 dB), the
# exponent-split "exact" form from there up.  Stated once, for the host proof of the gate (tests/test_prefilter_cpu.py) and for
# the GPU measurement of the map (tests/test_db_map_gpu.py), so that the two cannot drift apart.
P_EXACT_FROM = np.float32(1584.8932)   # SCN_P_EXACT_FROM
DB_MAP_ABS = 4.2e-6                    # dB: the product form's floor near 0 dB, where an ulp of the value vanishes
DB_MAP_ULP_FAST = 2.2                  # ulp of the value: the product form, below P_EXACT_FROM
DB_MAP_ULP_EXACT = 1.0                 # ulp of the value: the exact form, at and above P_EXACT_FROM


def _ulp32(db):
    return np.spacing(np.abs(np.asarray(db, np.float64)).astype(np.float32)).astype(np.float64)


def db_map_bound(db):
    """The product form's error bound in dB at a value near `db`, against the float64 value 5 log10 P (DESIGN.md section 3.1:
    max(4.2e-6 dB, 2.2 ulp of the value)).  It is the wider of the two halves, hence the one the gate is proved against."""
    return np.maximum(DB_MAP_ABS, DB_MAP_ULP_FAST * _ulp32(db))


def db_map_bound_exact(db):
    """The exact form's bound (powers >= P_EXACT_FROM, values from 16 dB up): 1.0 ulp of the value."""
    return DB_MAP_ULP_EXACT * _ulp32(db)


def db_map_bound_of_power(p, db):
    """The bound that applies to a bin of float power `p` whose float64 value is `db`: by the half of the map that p takes."""
    return np.where(np.asarray(p) >= P_EXACT_FROM, db_map_bound_exact(db), db_map_bound(db))


def db_to_power(db):
    """inverse of dB = 5*log10(P)  (utility.cpp:86-98 computes 10*log10 |X|)"""
    return np.power(10.0, np.asarray(db, np.float64) / 5.0)


def compare_spectra(db_test, db_ref):
    """Returns dict of error figures; raises AssertionError when outside the bar."""
    db_test = np.asarray(db_test, np.float64)
    db_ref = np.asarray(db_ref, np.float64)
    assert db_test.shape == db_ref.shape
    # NaN and +inf must sit in the same places.  -inf is an ordinary value of the map (a bin of exactly zero
    # power, utility.cpp:95): it enters the linear-power criterion as P = 0, so "-inf here, finite there" passes
    # only where the finite side is itself below 1e-5 of the buffer's mean power (cancellation residue -- e.g.
    # the constant 2e6-sized samples the negative-sum DC quirk produces leave bins of 0 vs 0.25 beside a 1e14
    # mean), and fails as a dB error wherever the reference bin is at or above the mean.
    bad_r = np.isnan(db_ref) | (db_ref == np.inf)
    bad_t = np.isnan(db_test) | (db_test == np.inf)
    assert np.array_equal(bad_r, bad_t), "nan / +inf pattern differs"
    ok_r, ok_t = np.isfinite(db_ref), np.isfinite(db_test)
    finite = ok_r & ok_t
    P_t = np.where(ok_t, db_to_power(np.where(ok_t, db_test, 0)), 0.0)
    P_r = np.where(ok_r, db_to_power(np.where(ok_r, db_ref, 0)), 0.0)
    mean = P_r.mean(axis=-1, keepdims=True)
    scale = np.maximum(P_r, mean)
    lin = np.where(bad_r, 0.0, np.abs(P_t - P_r) / np.where(scale > 0, scale, 1.0))
    big = ok_r & (P_r >= DB_MIN_POWER_RATIO * mean) & (mean > 0)
    with np.errstate(invalid="ignore"):
        db_err = np.where(ok_r & ok_t, np.abs(db_test - db_ref), np.where(ok_r == ok_t, 0.0, np.inf))
    db_bar = DB_REL * np.abs(db_ref) + DB_ABS
    with np.errstate(divide="ignore", invalid="ignore"):
        strict = np.where(P_r > 0, np.abs(P_t - P_r) / P_r, 0.0)
    out = {
        "max_rel_power_vs_max_bin_mean": float(lin.max()),
        "max_db_err_big_bins": float(db_err[big].max()) if big.any() else 0.0,
        "max_db_err_all_bins": float(db_err[finite].max()) if finite.any() else 0.0,
        "strict_per_bin_rel_power_max": float(strict.max()),
        "strict_per_bin_rel_power_p9999": float(np.quantile(strict, 0.9999)),
    }
    assert out["max_rel_power_vs_max_bin_mean"] <= REL_POWER, out
    assert np.all(db_err[big] <= db_bar[big]), out
    return out


def floor_errors(db_test, a64):
    """The third criterion: the bins compare_spectra is blind to -- those with a64^2 < REL_POWER * mean(a64^2), the floor under a
    strong signal -- in AMPLITUDE, relative to the buffer's rms level.  db_test [..., n]: the reported dB (10 log10 |X|); a64: the
    float64 DFT magnitude |X| of the same float32 samples.  Returns a dict:
      floor_err     max over the floor bins of (|a_t - a64| - (ln 10 / 10) * db_map_bound_of_power(a64^2, dB64) * a64) / rms, clamped at
                    0: a_t = 10^(dB / 10), rms = sqrt(mean a64^2) per buffer; the subtracted term is what the dB map's own proven
                    bound is worth in amplitude.  A transform's rounding error on ANY bin scales with the buffer's rms level, not with
                    the bin, so two correct float32 transforms give a few 1e-7 ... 1e-6 here (tests/test_dynamic_range_cpu.py
                    prints the table) whatever the bin holds.
      floor_share   the share of floor bins
      strict_p99    |a_t^2 - a64^2| / a64^2 at the 99th percentile of the floor bins (reported, never asserted)
      n_minus_inf   floor bins reported as -inf.  A -inf enters as a_t = 0, i.e. as the error a64 / rms: a caller's bound B so
                    accepts it exactly where a64 <= B * rms (plus the map's allowance).
    NaN and +inf are never acceptable, on any bin: AssertionError."""
    db_test = np.asarray(db_test, np.float64)
    a64 = np.asarray(a64, np.float64)
    assert db_test.shape == a64.shape and np.isfinite(a64).all() and (a64 >= 0).all()
    assert not np.isnan(db_test).any(), "NaN in a reported spectrum"
    assert not (db_test == np.inf).any(), "+inf in a reported spectrum"
    P = a64 * a64
    mean = P.mean(axis=-1, keepdims=True)
    rms = np.sqrt(mean)
    floor = P < REL_POWER * mean
    pos = a64 > 0
    d64 = 10.0 * np.log10(np.where(pos, a64, 1.0))
    allow = np.where(pos, (np.log(10.0) / 10.0) * db_map_bound_of_power(P, d64) * a64, 0.0)
    a_t = np.where(np.isfinite(db_test), np.power(10.0, np.where(np.isfinite(db_test), db_test, 0.0) / 10.0), 0.0)
    err = np.maximum(0.0, (np.abs(a_t - a64) - allow) / np.where(rms > 0, rms, 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        strict = np.where(pos, np.abs(a_t * a_t - P) / P, 0.0)
    return {
        "floor_err": float(err[floor].max()) if floor.any() else 0.0,
        "floor_share": float(floor.mean()),
        "strict_p99": float(np.quantile(strict[floor], 0.99)) if floor.any() else 0.0,
        "n_minus_inf": int((floor & np.isneginf(db_test)).sum()),
    }


def flip_unsafe(db_ref, threshold, margin=4.0):
    """Boolean mask (shape of db_ref): bins whose side of `threshold` the spectrum tolerance itself could change --
    |P_ref - P_thr| <= margin * REL_POWER * max(P_ref, mean P), or within GUARD_DB of the threshold in dB.  Hit
    lists are demanded bit-exact everywhere else.  (A buffer dominated by one huge component -- e.g. the 2e6-sized
    offset the negative-sum DC quirk of utility.cpp:77-78 adds -- leaves its other bins as cancellation residue far
    below the mean: two correct float32 FFTs then disagree by whole dB there.)"""
    db_ref = np.asarray(db_ref, np.float64)
    ok = np.isfinite(db_ref)
    P = np.where(ok, db_to_power(np.where(ok, db_ref, 0)), 0.0)
    mean = P.mean(axis=-1, keepdims=True)
    p_thr = db_to_power(threshold)
    lin = np.abs(P - p_thr) <= margin * REL_POWER * np.maximum(P, mean)
    with np.errstate(invalid="ignore"):
        near = np.abs(db_ref - threshold) < GUARD_DB
    return lin | near


def evaluated_mask(n, use_bandwidth=0.75, dc_ignore_bins=4):
    """Boolean [n] over natural bin j: True where process.cpp:46-52 evaluates the bin.  Walked over i with j = (i + n / 2) % n as
    the reference does: at odd n that map's inverse is i = (j + n - n / 2) % n, not (j + n / 2) % n, so a mask built from j (as this
    function did until tests/test_evaluated_mask_cpu.py) sat one bin off at 17, 1023, 4097, 65535; at even n the two agree."""
    half = n // 2
    use_window = int(use_bandwidth * n / 2.0)
    i = np.arange(n)
    j = (i + half) % n
    keep = ~((j < dc_ignore_bins) | ((n - j) < dc_ignore_bins) | (i < (half - use_window)) | (i > (half + use_window)))
    m = np.zeros(n, bool)
    m[j[keep]] = True
    return m


def pick_threshold(db_ref, n, start, use_bandwidth=0.75, dc_ignore_bins=4):
    """Smallest threshold >= start (steps of 0.01 dB) with an empty guard band on the
    reference spectrum, so bit-exact hit indices are a fair demand."""
    m = evaluated_mask(n, use_bandwidth, dc_ignore_bins)
    vals = np.asarray(db_ref, np.float64)[..., m].ravel()
    vals = np.sort(vals[np.isfinite(vals)])   # (sorted once: a step is two binary searches, also on 5 M bins)
    thr = np.float32(start)
    for _ in range(10000):
        lo = np.searchsorted(vals, float(thr) - GUARD_DB, side="right")    # first value > thr - GUARD
        hi = np.searchsorted(vals, float(thr) + GUARD_DB, side="left")     # first value >= thr + GUARD
        if lo >= hi:
            return float(thr)
        thr = np.float32(thr + np.float32(0.01))
    raise AssertionError("no guard-band-free threshold found")
