"""The detectors behind the transform -- the floor window (scn_floor_local.hip), the unit-wide floor (scn_floor.hip), the baseline
(scn_baseline.hip) -- and the averaged kernels' own mask sites (scn_average.hip), at the points of three axes their index arithmetic
depends on and the per-feature suites do not visit: the window's shape (guard mod 4, train mod 4, guard <= 2 or above), the mask
(use_bandwidth, dc_ignore_bins: a band that ends AT the spectrum's ends, a region of n records, bit 0 and the last bit of the signal
bitmap), and the sizes between the launchers' steps.  tests/detector_cases.py states the matrix and names the instantiation every
size reaches; tests/test_detector_cases_cpu.py holds it to the launchers.

Every comparison is an equality, bit for bit: the `_check` helpers of test_floor_gpu.py, test_local_floor_gpu.py and
test_baseline_gpu.py with their four assertions, against tests/floor_ref.py, local_floor_ref.py, baseline_ref.py and signals_ref.py.
Every case prints `geometry | case | instantiation | records compared` (profiles/detector_geometry.md is made of these lines)."""
import functools

import numpy as np
import pytest

from scanner_amd import Plan, capi
from tests import baseline_ref, floor_ref, local_floor_ref, signals_ref
from tests import detector_cases as dc
from tests import tolerances as tol
from tests.test_baseline_gpu import _check as baseline_check
from tests.test_baseline_gpu import _headers, _spectrum
from tests.test_floor_gpu import _check as floor_check
from tests.test_floor_gpu import _straddling, _submit
from tests.test_local_floor_gpu import _check as window_check

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS


def _mask_kw(mask):
    return dict(use_bandwidth=mask[0], dc_ignore_bins=mask[1])


def _evaluated_i(n, mask):
    """the evaluated fftshift indices, increasing"""
    return np.flatnonzero(tol.evaluated_mask(n, *mask)[(np.arange(n) + n // 2) % n])


@functools.lru_cache(maxsize=None)
def _input(n, nb, seed):
    """computed once per scene, shared and never written"""
    return _straddling(n, nb, seed)


def _report(case, instance, records):
    print(f"geometry | {case} | {instance} | {records}")


def _name(t):
    return "<" + ", ".join(("VEC" if v else "scalar") if isinstance(v, bool) else str(v) for v in t) + ">"


def _floor_name(n):
    t, kpt, reread = dc.floor_instance(n)
    return f"<{t}, {kpt}, {'re-read' if reread else 'registers'}>"


def _assert_every_bin(h, n, units, seq_units, what):
    """exactly n records per unit, i = 0 ... n - 1 in order"""
    assert len(h) == units * n, (what, len(h), units * n)
    assert np.array_equal(h["i"], np.tile(np.arange(n, dtype=np.uint32), units)), what
    assert np.array_equal(h["seq_id"], np.repeat(np.asarray(seq_units, np.uint64), n)), what


# ---- the window sweep: one plan per (n, mask), one submit per window ---------------------------------------------------------
@pytest.mark.parametrize("mask", [dc.DEFAULT_MASK, dc.FULL_MASK])
@pytest.mark.parametrize("n", dc.SWEEP_SIZES)
def test_window_sweep(built_lib, n, mask):
    """Every window of SWEEP on one spectrum + hits plan and one hits-only plan, set_floor_window between the submits: the list equals
    the reference's on the plan's own spectrum, the hits-only plan returns the same bytes.  A window that leaves an evaluated bin
    without a cell is refused with E_INVALID by both, and the next valid one is held like every other."""
    nb, threshold, trigger_count = dc.units_for(n), 1.0, n // 4
    x = _input(n, nb, n + 11)
    sub, fc_units, seq_units = _headers(nb, 1, capi.AVG_DWELL)
    kw = dict(max_batch=nb, detect=capi.DETECT_FLOOR, trigger_count=trigger_count, **_mask_kw(mask))
    evaluated = nb * _evaluated_i(n, mask).size
    refused, owed, records, first_p = [], False, 0, None  # owed: a refusal that no held window has followed yet
    with Plan(n, FS, threshold, flags=BOTH, **kw) as both, Plan(n, FS, threshold, flags=capi.OUT_HITS, **kw) as only:
        for window in dc.SWEEP:
            if not local_floor_ref.valid(n, *window, *mask):
                for plan in (both, only):
                    with pytest.raises(capi.ScannerError) as e:
                        plan.set_floor_window(*window)
                    assert e.value.status == capi.E_INVALID, window
                refused.append(window)
                owed = True
                continue
            out = []
            for plan in (both, only):
                plan.set_floor_window(*window)
                _submit(plan, 0, x, **sub)
                out.append(plan.collect(0))
                assert len(out[-1][1]) == plan.last_n_hits
            (p, h, t), (p2, h2, t2) = out
            first_p = p if first_p is None else first_p
            assert p.tobytes() == first_p.tobytes(), window  # the window moves no bin of the spectrum
            _, want_h, want_t = local_floor_ref.detect(p, threshold, *window, 0, fc_units, seq_units, FS, trigger_count, *mask)
            floor_ref.assert_same_records(h, want_h, f"n {n} mask {mask} window {window}")
            assert np.array_equal(t, want_t), window
            assert p2 is None and h2.tobytes() == h.tobytes() and np.array_equal(t2, t), window
            assert 0 < len(h) < evaluated, (window, len(h))
            records += len(h)
            owed = False
    assert sorted(refused) == sorted(dc.SWEEP_INVALID[(n, mask)])
    assert not owed  # each refusal was followed by a window that was held
    _report(f"window sweep n {n} mask {mask}: {len(dc.SWEEP) - len(refused)} windows, {len(refused)} refused", _name(dc.local_floor_instance(n)), records)


# ---- one window per (guard mod 4, train mod 4) at every instantiation and tile shape -----------------------------------------
RESIDUE_THRESHOLD = {0: 1.0, capi.FLOOR_MIN: 3.0, 1000: -1.0}  # offsets that leave both hits and non-hits at every rank (see below)


@pytest.mark.parametrize("window", dc.RESIDUES)
@pytest.mark.parametrize("mask", [dc.DEFAULT_MASK, dc.FULL_MASK])
@pytest.mark.parametrize("n", dc.RESIDUE_SIZES)
def test_window_residues(built_lib, n, mask, window):
    """The full _check of test_local_floor_gpu.py -- list, trigger, spectrum identical to the spectrum-only plan's, hits-only
    identical, host form -- at the median, and for the six windows at the limits also at the lowest and the highest rank.
    (|X|^2 of noise is exponential.  1.0 above the median of M cells: a hit with probability 0.34 ... 0.41.  3.0 above the minimum
    of M: a non-hit with probability 3.98 / (M + 3.98), 1.5 % at M = 256.  1.0 BELOW the maximum of M: a hit with probability about
    3 % at M = 256, more at fewer cells.)"""
    nb = dc.units_for(n)
    x = _input(n, nb, n + 13)
    evaluated = nb * _evaluated_i(n, mask).size
    permilles = [0] + ([capi.FLOOR_MIN, 1000] if window in dc.RESIDUES_EXTRA else [])
    for permille in permilles:
        p, h, t = window_check(n, x, RESIDUE_THRESHOLD[permille], window, permille, trigger_count=n // 4, **_mask_kw(mask))
        assert 0 < len(h) < evaluated, (permille, len(h), evaluated)
        _report(f"window residues n {n} mask {mask} window {window} permille {permille}", _name(dc.local_floor_instance(n)), len(h))


# ---- masks and sizes: the unit-wide floor and the baseline --------------------------------------------------------------------
UNIT_CASES = [(n, dc.DEFAULT_MASK) for n in dc.EDGE_SIZES] + [(n, m) for n in dc.MASK_SIZES for m in dc.OTHER_MASKS] + dc.EXTRA_UNIT_CASES


@pytest.mark.parametrize("n,mask", UNIT_CASES)
def test_floor_masks_and_sizes(built_lib, n, mask):
    nb = dc.units_for(n)
    evaluated = nb * _evaluated_i(n, mask).size
    if evaluated == 0:  # the mask lets no bin through: there is no rank to take
        with pytest.raises(capi.ScannerError) as e:
            Plan(n, FS, 1.0, max_batch=nb, detect=capi.DETECT_FLOOR, **_mask_kw(mask))
        assert e.value.status == capi.E_INVALID
        assert (n, mask) == (16, (0.5, 8))
        return
    p, fl, h = floor_check(n, _input(n, nb, n + 17), 1.0, trigger_count=n // 8, **_mask_kw(mask))
    assert 0 < len(h) < evaluated, (len(h), evaluated)
    _report(f"floor n {n} mask {mask}", _floor_name(n), len(h))


@pytest.mark.parametrize("n,mask", [c for c in UNIT_CASES if _evaluated_i(*c).size])
def test_baseline_masks_and_sizes(built_lib, n, mask):
    nb = dc.units_for(n)
    x, p_fixed = _spectrum(n, nb, seed=n + 19)
    _, baseline = _spectrum(n, nb, seed=n + 100019)  # an independent draw, a row per unit
    p, h = baseline_check(n, x, baseline, 0.0, want_spectrum=p_fixed, trigger_count=n // 8, **_mask_kw(mask))
    assert 0 < len(h) < nb * _evaluated_i(n, mask).size
    _report(f"baseline n {n} mask {mask}: {dc.baseline_loop_trips(n)} trips of the loop", _name(dc.baseline_instance(n)), len(h))


@pytest.mark.parametrize("n", dc.MASK_SIZES)
def test_full_mask_lists_every_bin(built_lib, n):
    """(1.0, 0), 200 below the floor and above a baseline of -inf: exactly n records per unit, i = 0 ... n - 1 in order -- a region
    of hit_region == n records, filled to its last slot"""
    nb = dc.units_for(n)
    seq_units = _headers(nb, 1, capi.AVG_DWELL)[2]
    p, fl, h = floor_check(n, _input(n, nb, n + 17), -200.0, trigger_count=n // 8, **_mask_kw(dc.FULL_MASK))
    assert np.isfinite(p).all()
    _assert_every_bin(h, n, nb, seq_units, f"floor n {n}")
    x, p_fixed = _spectrum(n, nb, seed=n + 19)
    p, hb = baseline_check(n, x, np.full((1, n), -np.inf, np.float32), -200.0, want_spectrum=p_fixed, trigger_count=n // 8,
                           **_mask_kw(dc.FULL_MASK))
    assert np.isfinite(p).all()
    _assert_every_bin(hb, n, nb, seq_units, f"baseline n {n}")
    _report(f"every bin n {n} mask {dc.FULL_MASK}: floor and baseline", f"{_floor_name(n)} {_name(dc.baseline_instance(n))}", len(h) + len(hb))


# ---- averaged plans: the accumulation kernel's and the combine kernel's own masks ---------------------------------------------
@pytest.mark.parametrize("mask", dc.AVERAGE_MASKS)
@pytest.mark.parametrize("G,K,split", dc.AVERAGE_ROUTES)
@pytest.mark.parametrize("n", dc.AVERAGE_SIZES)
def test_averaged_fixed_detector_masks(built_lib, n, G, K, split, mask):
    """200 below everything: per group exactly the mask's i, in order.  At the 0.9 quantile of the plan's own in-band spectrum: the
    list is mask & (own spectrum > threshold) -- the fixed decision restated as a baseline of that constant -- and the hits-only
    plan returns the same bytes."""
    nb, trigger_count = G * K, 100
    x = _input(n, nb, n + 23)
    sub, fc_units, seq_units = _headers(nb, K, capi.AVG_DWELL)
    kw = dict(max_batch=nb, average=K, trigger_count=trigger_count, **_mask_kw(mask))
    ev_i = _evaluated_i(n, mask)

    def run(threshold, flags):
        with Plan(n, FS, threshold, flags=flags, **kw) as plan:
            assert (plan.average_parts(nb) > 1) == split
            _submit(plan, 0, x, **sub)
            p, h, t = plan.collect(0)
            assert len(h) == plan.last_n_hits
            return p, h.copy(), t

    def want(p, threshold):
        return baseline_ref.detect(p, np.full((1, n), threshold, np.float32), 0, 0.0, fc_units, seq_units, FS, trigger_count, *mask)

    p, h, t = run(-200.0, BOTH)
    assert p.shape == (G, n) and np.isfinite(p).all()
    assert np.array_equal(h["i"], np.tile(ev_i.astype(np.uint32), G)) and np.array_equal(h["seq_id"], np.repeat(seq_units, ev_i.size))
    want_h, want_t = want(p, -200.0)
    baseline_ref.assert_same_records(h, want_h, f"n {n} mask {mask}: every evaluated bin")
    assert np.array_equal(t, want_t)
    records = len(h)
    threshold = float(np.float32(np.quantile(p[:, tol.evaluated_mask(n, *mask)], 0.9)))
    p2, h2, t2 = run(threshold, BOTH)
    assert p2.tobytes() == p.tobytes()
    want_h, want_t = want(p2, threshold)
    baseline_ref.assert_same_records(h2, want_h, f"n {n} mask {mask}: the 0.9 quantile")
    assert np.array_equal(t2, want_t) and 0 < len(h2) < G * ev_i.size
    p3, h3, t3 = run(threshold, capi.OUT_HITS)
    assert p3 is None and h3.tobytes() == h2.tobytes() and np.array_equal(t3, t2)
    _report(f"averaged fixed n {n} G {G} K {K} mask {mask}", "split route" if split else "in-workgroup route", records + 2 * len(h2))


def test_averaged_floor_full_mask(built_lib):
    n, (G, K, split) = dc.AVERAGE_DETECTOR_SIZES["floor"], dc.AVERAGE_ROUTES[0]
    p, fl, h = floor_check(n, _input(n, G * K, n + 29), 0.5, average=K, trigger_count=100, want_parts=split, **_mask_kw(dc.FULL_MASK))
    assert 0 < len(h) < G * n
    _report(f"averaged floor n {n} G {G} K {K} mask {dc.FULL_MASK}", _floor_name(n), len(h))


def test_averaged_window_full_mask(built_lib):
    n, (G, K, split) = dc.AVERAGE_DETECTOR_SIZES["window"], dc.AVERAGE_ROUTES[1]
    window = (27, 13)
    p, h, t = window_check(n, _input(n, G * K, n + 31), 0.2, window, average=K, trigger_count=100, want_parts=split, **_mask_kw(dc.FULL_MASK))
    assert 0 < len(h) < G * n
    _report(f"averaged window n {n} G {G} K {K} window {window} mask {dc.FULL_MASK}", _name(dc.local_floor_instance(n)), len(h))


def test_averaged_baseline_full_mask(built_lib):
    n, (G, K, split) = dc.AVERAGE_DETECTOR_SIZES["baseline"], dc.AVERAGE_ROUTES[0]
    x, p_fixed = _spectrum(n, G * K, seed=n + 37, average=K)
    _, baseline = _spectrum(n, G * K, seed=n + 100037, average=K)  # a row per group
    p, h = baseline_check(n, x, baseline, 0.0, want_spectrum=p_fixed, average=K, trigger_count=100, want_parts=split, **_mask_kw(dc.FULL_MASK))
    assert 0 < len(h) < G * n
    _report(f"averaged baseline n {n} G {G} K {K} mask {dc.FULL_MASK}", _name(dc.baseline_instance(n)), len(h))


# ---- signals and the compaction bitmap at full bandwidth ----------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.SIGNAL_SIZES)
def test_signals_at_full_bandwidth(built_lib, n):
    """(1.0, 0): bit 0 and bit n - 1 of a unit's bitmap are bins like any other.  Unit 0 carries a tone on natural bin n / 2, which
    is i = 0: its main lobe lies on i = 0 ... 3 and, across the spectrum's ends, on i = n - 3 ... n - 1 -- two signals, not one."""
    nb = dc.units_for(n)
    x = np.array(_input(n, nb, n + 41))
    x[0] += (0.5 * np.exp(2j * np.pi * (n // 2) * np.arange(n) / n)).astype(np.complex64)
    kw = dict(max_batch=nb, **_mask_kw(dc.FULL_MASK))
    with Plan(n, FS, -200.0, **kw) as plan:
        _submit(plan, 0, x)
        p, h, t = plan.collect(0)
        assert np.isfinite(p).all()
        _assert_every_bin(h, n, nb, np.arange(nb), f"n {n}: every bin")
        got = plan.collect_signals(0, 0)
    signals_ref.assert_same(got, signals_ref.signals(h, n, FS, 0), f"n {n}: every bin a hit")
    assert len(got) == nb and np.all(got["first_i"] == 0) and np.all(got["last_i"] == n - 1) and np.all(got["n_hits"] == n)
    assert np.array_equal(got["seq_id"], np.arange(nb))
    records = len(h)
    threshold = float(np.float32(np.median(p)))  # every bin is in band
    with Plan(n, FS, threshold, **kw) as plan:
        _submit(plan, 0, x)
        p2, h, t = plan.collect(0)
        assert p2.tobytes() == p.tobytes() and 0 < len(h) < nb * n
        want_h, want_t = baseline_ref.detect(p2, np.full((1, n), threshold, np.float32), 0, 0.0, None, None, FS, 1047, *dc.FULL_MASK)
        baseline_ref.assert_same_records(h, want_h, f"n {n}: the hits at the median")
        for gap in (0, 3):
            got = plan.collect_signals(0, gap)
            signals_ref.assert_same(got, capi.signals_from_hits(h, n, FS, gap), f"n {n} max_gap {gap}: GPU against scn_signals_from_hits")
            signals_ref.assert_same(got, signals_ref.signals(h, n, FS, gap), f"n {n} max_gap {gap}: GPU against the numpy reference")
            assert int(got["n_hits"].sum()) == len(h)
            assert np.any(got["first_i"] == 0), "no signal starts at i = 0"
            assert np.any(got["last_i"] == n - 1), "no signal ends at i = n - 1"
            unit0 = got[got["seq_id"] == 0]
            assert unit0[0]["first_i"] == 0 and unit0[-1]["last_i"] == n - 1 and len(unit0) >= 2  # the tone's two halves: no wrap
            records += len(got)
    _report(f"signals n {n} mask {dc.FULL_MASK}: hits at -200 + signals at the median, max_gap 0 and 3", f"{(n + 31) // 32} bitmap words", records + len(h))
