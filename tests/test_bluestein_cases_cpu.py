"""tests/bluestein_cases.py pinned on the host: the size list is what it claims, the bar (allowance_db) passes the fault-free numpy
Bluestein and FAILS each of the three float faults it exists for, and the bins it leaves to floor_errors are a negligible share of
every launch tests/test_bluestein_gpu.py runs.

MEASURED (test_the_bar_sees_every_float_fault, 8 buffers of dr_scenes.batch per size, Blackman-Harris; excess = the largest
|dB - dB64| / allowance_db over the held bins; the bar is 1):

      n     fault-free   float work buffers   float chirp   float filter transform
     17        0.049            9.0e+01          8.1e+01          1.4e+02
    257        0.067            5.2e+02          6.3e+02          4.7e+02
   1025        0.096            5.1e+03          5.8e+03          3.8e+03
   8191        0.090            5.9e+03          5.2e+03          3.5e+03
  40000        0.057            6.9e+03          8.8e+03          6.1e+03
  65535        0.065            1.1e+04          7.6e+03          7.4e+03

No fault stays inside the bar at any size: the smallest excess is 81 times the bar (8e-4 ... 0.14 dB on a floor bin against an
allowance of about 1e-5 dB).  The fault-free form sits below 0.1 because it forms the power in float64: of the bar's terms it
spends the two casts and numpy's own double error, none of the dB map's.  The excluded share of the GPU module's launches is
0 ... 3.1e-5 (test_excluded_share_of_every_gpu_launch prints each)."""
import numpy as np
import pytest

from scanner_amd import capi
from tests import bluestein_cases as bc
from tests import dr_scenes as sc
from tests import launch_caps as caps
from tests import tolerances as tol

WIRE_CASES, wire_id = bc.wire_cases(), bc.wire_id


def test_the_size_list_is_what_it_claims(built_lib, capsys):
    by_len = bc.check_sizes()
    assert bc.EDGE_SIZES == [17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049, 4095, 4097, 8191, 8193, 16383,
                             16385, 32767, 32769, 65535]
    assert all(n % 2 for n in bc.EDGE_SIZES) and all(n % 2 == 0 for n in bc.EVEN_SIZES)
    assert all(8191 % d for d in range(2, 91))                        # prime
    assert 40000 == 2 ** 6 * 5 ** 4 and capi.size_path(16000) == capi.PATH_FUSED   # 5-smooth, above the mixed-radix range
    # the transform lengths the suite never ran before this module, and the first pure radix-16 sequences of both parities
    for L in (7, 8, 9, 10, 12, 13):
        assert L in by_len
    assert caps.bluestein_radices(65) == caps.bluestein_radices(127) == [16, 16] and caps.bluestein_radices(1025) == [16, 16, 16]
    for group in (bc.WIRE_SIZES, bc.MODE_SIZES, bc.POSITION_SIZES, bc.SPECIAL_SIZES, bc.FAULT_SIZES):
        assert all(capi.size_path(n) == capi.PATH_BLUESTEIN for n in group), group
    assert "n = 65535: m = 2^17 stages [2, 16, 16, 16, 16]" in capsys.readouterr().out


def test_the_terms_are_what_the_docstring_derives():
    a64 = np.array([[1.0, 2.0 ** -20 * 0.999, 3.0, 1e-3]])
    rms = np.sqrt((a64 * a64).mean())
    t1, t2, t3 = bc.allowance_terms(a64)
    with np.errstate(divide="ignore"):
        assert np.array_equal(t1, tol.db_map_bound_of_power(a64 * a64, 10.0 * np.log10(a64)))
    assert bc.POWER_ROUNDINGS == 4 and np.all(t2 == (5.0 / np.log(10.0)) * 4 * 2.0 ** -24) and t2[0, 0] < 1e-6
    assert np.allclose(t3, (10.0 / np.log(10.0)) * 2.0 ** -40 * rms / a64, rtol=1e-15)
    assert np.array_equal(bc.allowance_db(a64), t1 + t2 + t3)
    assert bc.excluded(np.array([[1.0, 2.0 ** -20 * 0.5, 1.0, 1.0]])).tolist() == [[False, True, False, False]]
    # at the exclusion level the chain's term equals the map's floor; one float rounding of a work buffer is 2^16 times the chain's
    assert abs((10.0 / np.log(10.0)) * bc.CHAIN_EPS / bc.EXCLUDE_BELOW - tol.DB_MAP_ABS) < 0.1e-6
    assert 2.0 ** -24 / bc.CHAIN_EPS == 2.0 ** 16
    # the bar is three orders below the guard band of a picked threshold on every held bin
    assert (4.2e-6 * 2 + 5.2e-7) * 100 < tol.GUARD_DB


def test_the_numpy_tables_are_the_identity():
    """emulate() in complex128 IS the DFT: against numpy's FFT of the same samples, at sizes of both parities"""
    rng = np.random.default_rng(3)
    for n in (17, 18, 1002):
        x = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(np.complex64)
        X = np.fft.fft(x.astype(np.complex128), axis=-1)
        got = bc.emulate(x)
        assert np.abs(got - 5.0 * np.log10(X.real ** 2 + X.imag ** 2)).max() < 1e-5
        m, chirp, bf = bc.bluestein_tables(n)
        assert m == caps.bluestein_m(n) and chirp.shape == (n,) and bf.shape == (m,)


@pytest.mark.parametrize("n", bc.FAULT_SIZES)
def test_the_bar_sees_every_float_fault(oracle_mod, n):
    """the fault-free emulation passes allowance_db; float work buffers, a float chirp and a float filter transform each FAIL it"""
    x, _ = sc.batch(n, 8, seed=500)
    w = oracle_mod.Oracle(n).window()
    a64, _ = bc.owed(x, w)
    dbs = bc.float_faults(sc.windowed(x, w))
    clean = bc.check_spectrum(dbs[None], a64, f"n={n} fault-free")
    bc.floor_bound_check(dbs[None], a64, f"n={n} fault-free")
    line = f"n={n}: fault-free excess {clean['excess']:.3f} (excluded {clean['excluded_share']:.1e})"
    for fault in bc.FAULTS:
        fig = bc.measure_spectrum(dbs[fault], a64)
        line += f", {fault} {fig['excess']:.2e} ({fig['err_db']:.1e} dB)"
        with pytest.raises(AssertionError):
            bc.check_spectrum(dbs[fault], a64, f"n={n} {fault}")
        assert fig["excess"] > 1.0, (n, fault, fig)
    print(line)


@pytest.mark.parametrize("n,kind,enob,dc", WIRE_CASES, ids=[wire_id(*c) for c in WIRE_CASES])
def test_excluded_share_of_every_gpu_launch(oracle_mod, n, kind, enob, dc):
    """the bins allowance_db leaves to floor_errors (a64 < 2^-20 rms) are at most 1e-3 of every launch of the GPU module; and the
    launch owes records on both sides of its median count, so that its trigger flags can be of both kinds"""
    _, conv = bc.scene(oracle_mod, n, kind, enob, dc)
    assert conv.shape == (bc.count(n), n)
    a64, d64 = bc.owed(conv, oracle_mod.Oracle(n).window())
    share = float(bc.excluded(a64).mean())
    print(f"{wire_id(n, kind, enob, dc)}: {len(conv)} buffers, excluded share {share:.2e}")
    assert share <= bc.MAX_EXCLUDED_SHARE
    thr = bc.threshold_of(a64, d64, n)
    _, counts = bc.owed_hits(d64, n, thr, np.zeros(len(conv)), np.arange(len(conv)), 8000000)
    trig = bc.trigger_count_of(counts)
    assert (counts > trig).any() and (counts <= trig).any(), (thr, np.bincount(counts)[:8])
