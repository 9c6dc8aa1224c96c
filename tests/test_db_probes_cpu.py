"""The probe inputs of tests/db_probes.py, pinned on the host before any GPU is involved: every probe goes through numpy's float64
FFT and through the oracle (rectangular window, DC removal off).

Asserted:
  * the float64 spectrum holds the stated values: the flat probes exactly (a delta's transform is its amplitude), the line probes
    to the float64 FFT's own rounding (its twiddles cos(pi/2) etc. are ~1e-16, not 0: |X - stated| <= 64 eps N A), and exactly
    once rounded to float -- the stated values ARE floats;
  * the oracle's spectrum equals magnitude() of the stated values bit for bit, in all four wire formats;
  * exact_power is the float every formation of re^2 + im^2 gives (float product, fma, double sum rounded once), and the power
    ladder walks consecutive floats across SCN_P_EXACT_FROM -- which no REAL amplitude reaches;
  * the two figures the GPU test's knife-edge ladders rest on: sqrt(fl(a^2)) == |a|, and a ladder of 41 consecutive floats has
    41 distinct powers but only a handful of distinct correctly rounded dB values."""
import os

import numpy as np
import pytest

from tests import db_probes as pr
from tests import tolerances as tol

F32 = np.float32
SIZES = [16, 64, 512, 1000, 1024, 4096, 6000, 12000, 16384]
KINDS = [pr.KIND_FLOAT_COMPLEX, pr.KIND_SHORT_COMPLEX, pr.KIND_SHORT, pr.KIND_BYTE_COMPLEX]
NAMES = {pr.KIND_FLOAT_COMPLEX: "cfloat", pr.KIND_SHORT_COMPLEX: "int16", pr.KIND_SHORT: "int16planar", pr.KIND_BYTE_COMPLEX: "int8"}


def _oracle_db(oracle_mod, n, kind, raw):
    with oracle_mod.window_type(oracle_mod.WIN_RECTANGULAR):
        p, _, _ = oracle_mod.Oracle(n, 8000000, 1e9, kind=kind, enob=pr.ENOB[kind], correct_dc=False).run(raw, want_hits=False)
    return p


def _magnitude(oracle_mod, values):
    """the oracle's dB map (bit-pinned to the reference's utility.cpp) of real bin values"""
    v = np.ascontiguousarray(values, F32).reshape(-1)
    with np.errstate(divide="ignore"):
        return oracle_mod.Oracle(v.size).magnitude(v.astype(np.complex64)).reshape(np.shape(values))


def _to_complex(kind, raw, n):
    if kind == pr.KIND_FLOAT_COMPLEX:
        return raw.astype(np.complex128)
    q = raw.astype(np.float64) * pr.scale_of(kind)
    return (q[:, 0, :] + 1j * q[:, 1, :]) if kind == pr.KIND_SHORT else (q[:, :, 0] + 1j * q[:, :, 1])


@pytest.mark.parametrize("n", SIZES)
def test_flat_probes(oracle_mod, n):
    rng = np.random.default_rng(n)
    a = (np.exp2(rng.uniform(-60, 60, 40)) * rng.choice([-1.0, 1.0], 40)).astype(F32)
    amps = np.concatenate([a.astype(np.complex64), pr.power_ladder(tol.P_EXACT_FROM, 4, 4), pr.float_ladder(39.81072, 3, 3).astype(np.complex64)])
    x = pr.flat_raw(n, amps)
    X = np.fft.fft(x.astype(np.complex128), axis=1)
    assert np.array_equal(X, np.repeat(amps.astype(np.complex128)[:, None], n, axis=1)), "a delta's float64 transform is its amplitude"
    # the oracle forms sqrtf(re*re + im*im) in float and maps that: equal to magnitude() of the stated bins by construction of
    # the comparison, and to the float64 value of the exact power within half an ulp plus the sqrtf step's own rounding
    want = pr.flat_raw(1, amps)[:, 0]
    m = oracle_mod.Oracle(len(want)).magnitude(want)
    p = _oracle_db(oracle_mod, n, pr.KIND_FLOAT_COMPLEX, x)
    assert p.tobytes() == np.repeat(m[:, None], n, axis=1).tobytes()
    real = amps.imag == 0
    d = pr.db64(pr.exact_power(amps))
    assert (np.abs(m[real].astype(np.float64) - d[real]) <= 0.5 * np.spacing(np.abs(d[real]).astype(F32)) + 1.4e-7).all()


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
@pytest.mark.parametrize("n", SIZES)
def test_line_probes(oracle_mod, n, kind):
    i1, i3, ia = pr.line_params(kind, n, 24)
    raw = pr.pack(kind, pr.line_ints(n, i1, i3, ia))
    want = pr.line_spectrum(kind, n, i1, i3, ia)
    X = np.fft.fft(_to_complex(kind, raw, n), axis=1)
    top = float(np.abs(want).max())
    assert np.abs(X - want.astype(np.float64)).max() <= 64 * np.finfo(np.float64).eps * top
    assert np.array_equal(X.real.astype(F32), want) and np.abs(X.imag).max() <= 64 * np.finfo(np.float64).eps * top
    p = _oracle_db(oracle_mod, n, kind, raw)
    assert p.tobytes() == _magnitude(oracle_mod, want).tobytes(), "the oracle's spectrum is magnitude() of the stated bins"
    # the floor of a line probe is the flat probe of the same amplitude (an impulse of ia quanta), in every wire format
    flat = pr.pack(kind, pr.line_ints(n, 0 * ia, 0 * ia, ia))
    pf = _oracle_db(oracle_mod, n, kind, flat)
    floor = np.ones(n, bool)
    floor[[n // 4, 3 * n // 4]] = False
    assert p[:, floor].tobytes() == pf[:, floor].tobytes()


def test_exact_power_is_every_formation():
    amps = np.concatenate([pr.power_ladder(tol.P_EXACT_FROM, 40, 40), pr.power_ladder(F32(3.0e9), 20, 20), pr.power_ladder(F32(400.0), 20, 20)])
    p = pr.exact_power(amps)
    re, im = amps.real.astype(np.float64), amps.imag.astype(np.float64)
    assert np.array_equal(p, (re * re + im * im).astype(F32)), "the double sum, rounded once"
    assert np.array_equal(p, ((amps.real * amps.real).astype(np.float64) + im * im).astype(F32)), "fma(im, im, fl(re * re))"
    lad = pr.exact_power(pr.power_ladder(tol.P_EXACT_FROM, 40, 40))
    assert lad[40] == tol.P_EXACT_FROM and (np.diff(lad.view(np.uint32).astype(np.int64)) == 1).all()
    # no real amplitude has the power SCN_P_EXACT_FROM: the reason the ladder is complex
    near = pr.float_ladder(np.sqrt(float(tol.P_EXACT_FROM)), 8, 8)
    assert tol.P_EXACT_FROM not in pr.exact_power(near.astype(np.complex64))


def test_the_figures_the_ladders_rest_on(oracle_mod):
    rng = np.random.default_rng(7)
    a = np.exp2(rng.uniform(-60, 60, 1000000)).astype(F32)
    assert np.array_equal(np.sqrt(a * a), a), "sqrtf(fl(a^2)) returns the amplitude itself"
    lad = pr.float_ladder(60.0, 20, 20)
    p = pr.exact_power(lad.astype(np.complex64))
    db = oracle_mod.Oracle(41).magnitude(lad.astype(np.complex64))
    assert len(np.unique(p)) == 41 and 3 <= len(np.unique(db)) <= 8
    mid = db[20]
    assert (db == mid).sum() >= 2 and (db > mid).any() and (db < mid).any()


def test_shared_bound_values():
    """the figures of DESIGN.md section 3.1, as the prefilter proof and the GPU measurement both import them"""
    assert tol.db_map_bound(0.0) == 4.2e-6 and tol.db_map_bound(1e-3) == 4.2e-6
    assert tol.db_map_bound(15.0) == 4.2e-6 and tol.db_map_bound(-100.0) == 2.2 * float(np.spacing(F32(100.0)))
    assert tol.db_map_bound_exact(40.0) == float(np.spacing(F32(40.0)))
    assert np.array_equal(tol.db_map_bound_of_power(np.array([1584.0, 1584.8932, 1e6], F32), np.array([15.99, 16.0, 30.0])),
                          [tol.db_map_bound(15.99), tol.db_map_bound_exact(16.0), tol.db_map_bound_exact(30.0)])
    assert tol.P_EXACT_FROM.view(np.uint32) == 0x44C61C95


def test_design_names_this_suite():
    """DESIGN.md sections 3.1 and 4 name the three files by their bare names (they live beside this one), and they exist"""
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(os.path.dirname(here), "DESIGN.md")).read()
    for name in ("test_db_map_gpu.py", "db_probes.py", "test_db_probes_cpu.py"):
        assert f"`{name}`" in txt and os.path.exists(os.path.join(here, name)), name
