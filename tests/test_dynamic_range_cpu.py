"""The high-dynamic-range scenes of tests/dr_scenes.py and the floor metric of tests/tolerances.py floor_errors, pinned on the host
(no GPU): what tests/test_dynamic_range_gpu.py holds the kernels to has to be true of the inputs and of the yardstick first.

  * the scenes are what they claim: the share of floor bins (power below REL_POWER of the buffer's mean -- the bins
    compare_spectra cannot see) is >= 0.85 from 64 points up and >= 0.95 from 1000 up, and pinned to the float64 figure at 16, 17
    and 32 points, where the blocker's main lobe is half the spectrum; the blocker's peak over the mean is what a Blackman-Harris
    tone gives; the weak tones stand over the median floor by at least weak_excess_db() less 1 dB;
  * the metric: zero on the float64 spectrum itself; -inf counted as the bin's whole amplitude; NaN and +inf refused;
  * the gap it closes: a -120 dBc spur on ONE floor bin of a correct float32 spectrum exceeds 2 Y while compare_spectra passes;
  * the yardstick Y per size of the GPU module (printed: run with -s or -rP), the larger floor_errors figure of the oracle's chain
    through Oracle.run in its default mode and of scipy.fft on complex64.  THE ORACLE'S DEFAULT MODE IS NO FLOAT32 TRANSFORM in
    this metric: it accumulates in double and rounds once (oracle/scn_oracle.c), its figure is 0 at every size -- within the dB
    map's allowance of float64 -- so Y is pocketfft's figure and the oracle's default mode cannot say whether that is an outlier
    (asserted below as figure <= 1e-8, so that a change of the oracle's mode is noticed).  The outlier check is therefore made
    against the oracle's float32 FFT proper, its textbook radix-2 in float (oracle.set_fft_mode(False)): that and pocketfft stay
    within 2x of each other at every power of two of the GPU module.  It does not enter Y.  At the other lengths the oracle
    computes in double and scipy alone supplies the yardstick.

Measured here (cfloat, the GPU module's launch shapes, this module's seed): Y = 3.1e-7 at 16 points, 5.2e-7 at 64, 1.8e-6 at 1024,
3.7e-6 at 4096, 4.5e-6 at 16384, 1.1e-5 at 65536; radix-2 float / pocketfft between 0.7 and 1.7.  Y is a maximum over the floor bins of
a launch and moves by up to 2x with the draw: the GPU module's seeds give 2.8e-6 at 4096 and 6.2e-6 ... 9.5e-6 at 65536
(profiles/dynamic_range.txt), which is why it is measured per launch on the very buffers and never tabulated."""
import numpy as np
import pytest

from scanner_amd import capi
from tests import dr_scenes as sc
from tests import tolerances as tol

CF = capi.KIND_FLOAT_COMPLEX
SCENE_SIZES = [16, 17, 32, 64, 128, 256, 512, 1000, 1024, 4096, 6000, 12000, 16384, 20000, 65535, 65536]


def _count(n):
    return max(2, (1 << 18) // n) + (37 if n <= 512 else 0)


def _scene(oracle_mod, n, kind=CF, enob=12, dc=False, seed=1):
    x, info = sc.batch(n, _count(n), seed)
    raw = sc.to_wire(x, kind, enob, dc)
    conv = sc.convert(oracle_mod, n, kind, enob, dc, raw)
    w = oracle_mod.Oracle(n).window()
    return raw, conv, w, np.sqrt(sc.ref64_power(conv, w)), info


@pytest.mark.parametrize("n", SCENE_SIZES)
def test_the_scenes_are_what_they_claim(oracle_mod, n):
    raw, conv, w, a64, info = _scene(oracle_mod, n)
    w = w.astype(np.float64)
    with np.errstate(divide="ignore"):
        fig = tol.floor_errors(10.0 * np.log10(a64), a64)
    share = fig["floor_share"]
    sc.assert_floor_share(n, share)
    P = a64 * a64
    # the blocker: a tone of amplitude A under window w peaks at (A sum(w) S)^2, S the scalloping (1 on a bin centre, 0.909 half way
    # between two with Blackman-Harris); the buffer's mean power is A^2 sum(w^2) by Parseval, the noise adds 3e-7 of it
    R = w.sum() ** 2 / (w * w).sum()
    ratio = P.max(axis=1) / P.mean(axis=1)
    assert (ratio >= 0.80 * R).all() and (ratio <= 1.02 * R).all(), (n, float(ratio.min()) / R, float(ratio.max()) / R)
    peak = P.argmax(axis=1)
    assert (np.abs((peak - sc.signed_to_natural(info["f_blocker"], n) + n // 2) % n - n // 2) <= 1).all(), "the blocker is where the scene says"
    if n >= 64:
        floor = P < tol.REL_POWER * P.mean(axis=1, keepdims=True)
        rms_noise = np.median(a64[floor]) / np.sqrt(np.log(2.0))    # a noise bin's amplitude is Rayleigh: median = rms sqrt(ln 2)
        # (within 15 %: at 64 points the weak tones' 3 bins and the skirt of the main lobe are a tenth of the 56 floor bins and lift the
        #  median by 10 %; from 256 points up it is within 2 %)
        assert abs(rms_noise / (sc.SIGMA * np.sqrt(2.0 * (w * w).sum())) - 1.0) < (0.15 if n < 256 else 0.03), "the floor is the noise"
        checked = 0
        for f, db in zip(info["f_weak"], sc.WEAK_DB):
            E = sc.weak_excess_db(n, w, db)
            if E < 6.0:
                continue     # a tone under the floor: present, but nothing can be said of its bin
            got = 10.0 * np.log10(np.median(a64[:, sc.signed_to_natural(f, n)]) / rms_noise)
            assert got >= E - 1.0, (n, db, got, E)
            checked += 1
        assert checked >= 1
    print(f"n={n}: {len(a64)} buffers, floor share {share:.4f}, peak / mean {ratio.mean():.1f} ({ratio.mean() / R:.3f} of a centred tone's)")


def test_the_metric_on_float64_and_on_special_values():
    rng = np.random.default_rng(3)
    a = np.abs(rng.standard_normal((3, 256))) * 1e-3
    a[:, 17] = 40.0
    d = 10.0 * np.log10(a)
    fig = tol.floor_errors(d, a)
    assert fig["floor_err"] == 0.0 and fig["strict_p99"] < 1e-12 and fig["n_minus_inf"] == 0 and fig["floor_share"] > 0.9
    # the dB map's allowance: a value at the bound passes, one at three times the bound shows
    b = tol.db_map_bound_of_power(a * a, d)
    assert tol.floor_errors(d + 0.999 * b, a)["floor_err"] == 0.0
    assert tol.floor_errors(d + 3.0 * b, a)["floor_err"] > 0.0
    # -inf is the bin's whole amplitude
    e = d.copy()
    e[1, 5] = -np.inf
    fig = tol.floor_errors(e, a)
    rms = np.sqrt((a[1] ** 2).mean())
    assert fig["n_minus_inf"] == 1 and abs(fig["floor_err"] - a[1, 5] / rms) < 1e-6 * a[1, 5] / rms
    for bad in (np.nan, np.inf):
        e = d.copy()
        e[2, 9] = bad
        with pytest.raises(AssertionError):
            tol.floor_errors(e, a)
    # a zero bin reported as -inf is exact
    z = a.copy()
    z[0, 3] = 0.0
    with np.errstate(divide="ignore"):
        assert tol.floor_errors(10.0 * np.log10(z), z)["floor_err"] == 0.0


@pytest.mark.parametrize("n", [64, 1024, 4096, 16384, 65536])
def test_a_spur_under_the_blocker_is_seen_by_the_floor_metric_only(oracle_mod, n):
    """-120 dBc (1e-6 of the blocker's amplitude) on one floor bin of pocketfft's own float32 spectrum"""
    raw, conv, w, a64, _ = _scene(oracle_mod, n)
    dbs = sc.float32_dbs(oracle_mod, n, CF, 12, False, raw, conv, w)
    Y, _ = sc.yardstick(tol, dbs, a64)
    d64 = 10.0 * np.log10(a64)
    clean = dbs["pocketfft"].astype(np.float64)
    assert tol.floor_errors(clean, a64)["floor_err"] <= Y
    tol.compare_spectra(clean, d64)
    P = a64 * a64
    floor = P < tol.REL_POWER * P.mean(axis=1, keepdims=True)
    b = 1
    j = int(np.flatnonzero(floor[b] & tol.evaluated_mask(n))[len(a64) % 7])
    spur = 1e-6 * a64[b].max()
    spurred = clean.copy()
    spurred[b, j] = np.float32(10.0 * np.log10(10.0 ** (clean[b, j] / 10.0) + spur))
    fig = tol.floor_errors(spurred, a64)
    tol.compare_spectra(spurred, d64)            # the existing bar does not see it ...
    assert fig["floor_err"] > 2.0 * Y, (fig, Y)  # ... the floor criterion does
    rms = np.sqrt(P[b].mean())
    print(f"n={n}: spur {spur / rms:.2e} of the rms level on bin {j} (itself {a64[b, j] / rms:.2e}): floor_err {fig['floor_err']:.2e} > 2 Y = {2 * Y:.2e}; "
          f"compare_spectra passes ({spur * (2 * a64[b, j] + spur) / P[b].mean():.1e} of the mean power against the bar's 1e-5)")


def test_yardstick_per_size(built_lib, oracle_mod):
    rows = []
    for n in sc.spectrum_sizes():
        raw, conv, w, a64, _ = _scene(oracle_mod, n)
        Y, each = sc.yardstick(tol, sc.float32_dbs(oracle_mod, n, CF, 12, False, raw, conv, w), a64)
        assert 1e-7 < Y < 3e-5, (n, Y)       # a float32 transform: a few ulp of the rms level, growing like sqrt(log n) ... sqrt(n)
        row = f"{n:6d}  Y {Y:.2e}  pocketfft {each['pocketfft']:.2e}"
        if "oracle" in each:
            assert each["oracle"] <= 1e-8, (n, each)
            oracle_mod.set_fft_mode(False)
            try:
                p0 = oracle_mod.Oracle(n, 8000000, 1e9).run(raw, want_hits=False, threads=8)[0]
            finally:
                oracle_mod.set_fft_mode(True)
            r2 = tol.floor_errors(p0, a64)["floor_err"]
            assert r2 <= 2.0 * each["pocketfft"] and each["pocketfft"] <= 2.0 * r2, (n, r2, each)
            row += f"  oracle (default mode) {each['oracle']:.1e}  oracle (radix-2 float) {r2:.2e}  ratio {r2 / each['pocketfft']:.2f}"
        rows.append(row)
    print("points  yardstick of the floor criterion (cfloat scene, the GPU module's launch shape)\n" + "\n".join(rows))
