"""The sweep trace on the GPU (scn_plan_set_trace, scn_plan_update_trace, scn_plan_get_trace; scn_trace.hip).  Every assertion is an
equality of bits: max_db and min_db as uint32, count as uint64, EVERY cell of every case -- the empty ones must read (-inf, +inf, 0).
tests/trace_ref.py, the numpy model written from the definition, is fed the spectrum and the centres the plan itself returned: the
fold is a pure function of them (integers and compares only), so there is no tolerance and nothing exempt.  capi.trace_fold_spectrum,
the host form, is held to the same bits beside it.

One submit per case, then one scn_plan_set_trace + scn_plan_update_trace per geometry (set_trace resets; a collected slot may be
folded any number of times).  The geometries are those of tests/test_trace_cpu.py: cell_hz in {bin_step, bin_step + 1, 64 bin_step +
7, three sample rates, 1}, f0 inside the first unit's band, the last cell ending inside the last unit's."""
import ctypes as C

import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi, synth
from tests import launch_caps, trace_caps, trace_ref
from tests.test_floor_gpu import _noise, _straddling, _submit
from tests.test_trace_cpu import geometries

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS
QUIET = dict(threshold=1e9)  # a fixed threshold nothing exceeds: the trace does not depend on the hits


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.ScannerError as e:
        return e.status
    return capi.OK


def _centres(units, step=6e6, first=100e6 + 0.5):
    """centres with a fraction -- the double addition and the cast per bin -- and, every other unit, a whole number of hertz, whose
    cells the kernel takes from integers alone (scn_trace_unit)"""
    fc = first + step * np.arange(units)
    fc[1::2] = np.floor(fc[1::2])
    return fc


def _check_trace(plan, want, what):
    got = plan.trace()
    assert trace_ref.same(got, want), (what, trace_ref.describe(got, want))
    return got


def _fold_geometries(plan, slot, p, centres, what, geoms=None, sample_rate=FS, **mask):
    """for each geometry: a fresh trace, the slot folded once, every cell against the model and the host form; returns the cells folded"""
    folded = 0
    for f0, cell_hz, cells in geoms or geometries(plan.n, centres):
        plan.set_trace(f0, cell_hz, cells)
        _check_trace(plan, trace_ref.new(cells), (what, "reset"))
        plan.update_trace(slot)
        want = trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, sample_rate, centres, **mask)
        _check_trace(plan, want, (what, f0, cell_hz, cells))
        host = capi.trace_init(cells)
        capi.trace_fold_spectrum(host, f0, cell_hz, p, sample_rate, centres, **mask)
        assert trace_ref.same(host, want), (what, "host form", cell_hz)
        folded += int(want[2].sum())
    assert folded > 0, (what, "no geometry folded a bin")
    return folded


# team of 64 (a wave per unit, several units per workgroup): 16 and 512 by 16-byte loads (1 and 2 in flight), 18 by 4-byte loads (rows
# 8-byte aligned); team of 256: 1024 and 4096 by 16-byte loads (1 and 4 in flight), 1001 by 4-byte loads; team of 1024: 8192 and 65536
# by 16-byte loads (2 and 4 in flight), 4098 by 4-byte loads
@pytest.mark.parametrize("n,units", [(16, 7), (18, 5), (512, 6), (1001, 3), (1024, 5), (4096, 4), (4098, 3), (8192, 3), (65536, 2)])
def test_sizes_teams_and_load_forms(built_lib, n, units):
    centres = _centres(units)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _noise(n, units, seed=n), center_freqs=centres)
        p = plan.collect(0)[0]
        assert np.isfinite(p).all()
        _fold_geometries(plan, 0, p, centres, f"n {n}")


@pytest.mark.parametrize("scene", ["overlapping", "repeated", "negative_start"])
@pytest.mark.parametrize("n", [16, 1024])
def test_centres_that_share_cells_or_wrap(built_lib, n, scene):
    centres = {"overlapping": 100e6 + 5e6 * np.arange(4), "repeated": np.array([100e6, 100e6, 106e6, 100e6]),
               "negative_start": np.array([1e6, 3e6, 9e6, 2e6])}[scene]
    with Plan(n, FS, max_batch=4, **QUIET) as plan:
        _submit(plan, 0, _noise(n, 4, seed=n + 1), center_freqs=centres)
        p = plan.collect(0)[0]
        _fold_geometries(plan, 0, p, centres, (n, scene))
        if scene == "negative_start":  # the wrapped bins are found by a grid up there, and by none down here
            f = trace_ref.bin_freqs(n, FS, centres[0])
            assert f[0] == (1 << 64) - 3000000
            bs = FS // n
            _fold_geometries(plan, 0, p, centres, (n, scene, "wrapped"), geoms=[((1 << 64) - 3000000, bs, 3000000 // bs), (0, 64 * bs, 40)])


def test_int16_input(built_lib):
    n, units = 1024, 5
    centres = _centres(units)
    raw = synth.quantize(synth.cfloat_batch(n, units, seed=3), capi.KIND_SHORT_COMPLEX)
    with Plan(n, FS, kind=capi.KIND_SHORT_COMPLEX, enob=12, correct_dc=True, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, raw, nb=units, center_freqs=centres)
        _fold_geometries(plan, 0, plan.collect(0)[0], centres, "int16")


def test_sample_rate_below_n(built_lib):
    """bin_step = 0: every bin of a unit carries fc - sample_rate / 2, the whole unit falls into one cell"""
    n, fs, centres = 16, 10, np.array([1000.0, 1007.0, 1000.0])
    with Plan(n, fs, max_batch=3, **QUIET) as plan:
        _submit(plan, 0, _noise(n, 3, seed=8), center_freqs=centres)
        p = plan.collect(0)[0]
        _fold_geometries(plan, 0, p, centres, "bin_step 0", geoms=[(990, 10, 2), (995, 1, 8), (996, 1, 8)], sample_rate=fs)
        plan.set_trace(990, 10, 2)
        plan.update_trace(0)
        assert plan.trace()[2].tolist() == [12, 6]  # 995 twice, 1002 once: six evaluated bins each


def test_mask_of_the_plan(built_lib):
    n, units = 64, 3
    centres = _centres(units)
    for mask in (dict(dc_ignore_bins=0), dict(dc_ignore_bins=9, use_bandwidth=0.5), dict(use_bandwidth=1.0, dc_ignore_bins=1)):
        with Plan(n, FS, max_batch=units, **QUIET, **mask) as plan:
            _submit(plan, 0, _noise(n, units, seed=4), center_freqs=centres)
            _fold_geometries(plan, 0, plan.collect(0)[0], centres, mask, **mask)


def test_indexed_submit_that_wraps_the_table(built_lib):
    n, units, first = 512, 5, 3
    table = 100e6 + 6e6 * np.arange(units + 2)
    centres = table[(first + np.arange(units)) % table.size]  # entries 3 4 5 6 0
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        plan.set_table(table)
        _submit(plan, 0, _noise(n, units, seed=5), first_index=first)
        p = plan.collect(0)[0]
        lo = int(table[0] - FS / 2)
        _fold_geometries(plan, 0, p, centres, "indexed", geoms=[(lo + 1000000, FS // n + 1, 2000), (lo, 64 * (FS // n) + 7, 50), (lo, 3 * FS, 20)])


@pytest.mark.parametrize("layout", [capi.AVG_DWELL, capi.AVG_SWEEPS])
def test_averaged_plan(built_lib, layout):
    n, k, groups = 1024, 4, 3
    centres = _centres(groups)
    fc = np.repeat(centres, k) if layout == capi.AVG_DWELL else np.tile(centres, k)
    with Plan(n, FS, max_batch=k * groups, average=k, average_layout=layout, **QUIET) as plan:
        _submit(plan, 0, _noise(n, k * groups, seed=6), center_freqs=fc)
        p = plan.collect(0)[0]
        assert p.shape == (groups, n)
        _fold_geometries(plan, 0, p, centres, ("averaged", layout))


@pytest.mark.parametrize("detect", [capi.DETECT_FLOOR, capi.DETECT_BASELINE])
@pytest.mark.parametrize("n", [64, 4096])
def test_hits_only_detector_plans_against_their_twins(built_lib, n, detect):
    """a floor / baseline plan flagged hits-only keeps the spectrum its detect kernel reads in a buffer of its own: the trace folded
    from it must be the trace of the SPECTRUM|HITS twin on the same input -- both run the spectrum-only transform"""
    units = 4
    centres = _centres(units)
    x = _straddling(n, units, seed=n + 7)
    kw = dict(threshold=0.0, detect=detect, max_batch=units)
    if detect == capi.DETECT_BASELINE:
        kw["baseline"] = units
    traces = {}
    for flags in (BOTH, capi.OUT_HITS):
        with Plan(n, FS, flags=flags, **kw) as plan:
            _submit(plan, 0, x, center_freqs=centres)
            p = plan.collect(0)[0]
            traces[flags] = []
            for f0, cell_hz, cells in geometries(n, centres):
                plan.set_trace(f0, cell_hz, cells)
                plan.update_trace(0)
                traces[flags].append(plan.trace())
                if flags == BOTH:
                    want = trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, FS, centres)
                    assert trace_ref.same(traces[flags][-1], want), (n, detect, cell_hz, trace_ref.describe(traces[flags][-1], want))
                    assert int(want[2].sum()) > 0
    for a, b in zip(traces[BOTH], traces[capi.OUT_HITS]):
        assert trace_ref.same(b, a), (n, detect, trace_ref.describe(b, a))


def test_spectrum_in_the_callers_buffer(built_lib):
    n, units = 1024, 4
    centres = _centres(units)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        d_power = torch.full((units, n), float("nan"), dtype=torch.float32, device="cuda")
        _submit(plan, 0, _noise(n, units, seed=9), center_freqs=centres, d_power_db=d_power)
        plan.collect(0, want_power=False)
        torch.cuda.synchronize()
        p = d_power.cpu().numpy()
        assert np.isfinite(p).all()
        _fold_geometries(plan, 0, p, centres, "d_power_db")


@pytest.mark.parametrize("n,units", [(16, 6), (18, 4), (1024, 3)])
def test_cell_mapping_against_the_records(built_lib, n, units):
    """a fixed threshold below every finite dB value makes every evaluated finite bin a hit: the trace the model folds from the hit
    list -- each record's own freq_hz and power_db -- must be the GPU's trace, cell by cell"""
    centres = np.concatenate([[1e6], _centres(units - 1, step=5e6)])  # one negative start, then overlapping bands
    with Plan(n, FS, threshold=-1e30, max_batch=units) as plan:
        _submit(plan, 0, _noise(n, units, seed=n + 11), center_freqs=centres)
        p, hits, _ = plan.collect(0)
        ev = trace_ref.evaluated(n)
        band = p[:, (np.arange(n) + n // 2) % n][:, ev]
        assert np.isfinite(band).all(), "an evaluated bin is -inf or NaN: it would be no hit"
        assert len(hits) == band.size
        for f0, cell_hz, cells in geometries(n, centres) + [(0, 64 * (FS // n), 400)]:
            plan.set_trace(f0, cell_hz, cells)
            plan.update_trace(0)
            want = trace_ref.fold_hits(trace_ref.new(cells), f0, cell_hz, hits)
            _check_trace(plan, want, ("from the records", n, cell_hz))
            assert trace_ref.same(want, trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, FS, centres))


def test_special_values(built_lib):
    n, units = 64, 3
    centres = _centres(units)
    x = _noise(n, units, seed=12)
    x[1] = 0  # |X| = 0 everywhere: -inf in every bin, counted
    x[2, 5] = np.float32(np.nan) + 0j  # one NaN sample: the whole unit is NaN and contributes nothing
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, x, center_freqs=centres)
        p = plan.collect(0)[0]
        assert np.all(np.isneginf(p[1])) and np.all(np.isnan(p[2])) and np.isfinite(p[0]).all()
        _fold_geometries(plan, 0, p, centres, "specials")
        lo = int(centres[1] - FS / 2)
        plan.set_trace(lo, FS, 1)  # unit 1's band alone
        plan.update_trace(0)
        mx, mn, ct = plan.trace()
        inside = trace_ref.bin_freqs(n, FS, centres[0])[trace_ref.evaluated(n)] >= lo
        assert ct[0] == int(trace_ref.evaluated(n).sum()) + int(inside.sum())
        assert np.isneginf(mn[0])
        plan.set_trace(int(centres[2] - FS / 2 + 2000000), FS, 1)  # beyond unit 1's band: the NaN unit alone
        plan.update_trace(0)
        _check_trace(plan, trace_ref.new(1), "a NaN unit")


def test_accumulation_reset_and_windows(built_lib):
    n, units = 512, 4
    centres = [_centres(units), _centres(units, first=103e6), _centres(units, first=98e6 + 0.25)]
    f0, cell_hz, cells = 97000000, 40 * (FS // n) + 3, 60
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        plan.set_trace(f0, cell_hz, cells)
        want = trace_ref.new(cells)
        for k, slot in enumerate((0, 1, 0)):  # two slots, three submits
            _submit(plan, slot, _noise(n, units, seed=20 + k), center_freqs=centres[k])
            p = plan.collect(slot)[0]
            plan.update_trace(slot)
            want = trace_ref.fold(want, f0, cell_hz, p, FS, centres[k])
            _check_trace(plan, want, ("accumulated", k))
        twice = trace_ref.fold(want, f0, cell_hz, p, FS, centres[2])  # the same slot again: counts twice, max and min stay
        plan.update_trace(0)
        got = _check_trace(plan, twice, "folded twice")
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert got[2].sum() > want[2].sum()
        # windows of the read-out, and its range check
        for first, count in ((0, cells), (7, 13), (cells - 1, 1), (cells, 0), (0, 0)):
            win = plan.trace(first, count)
            assert trace_ref.same(win, tuple(a[first:first + count] for a in twice)), (first, count)
        for first, count in ((0, cells + 1), (cells, 1), (cells + 1, 0), (0xFFFFFFFF, 2)):
            assert _status(plan.trace, first, count) == capi.E_INVALID, (first, count)
        only_count = np.zeros(5, np.uint64)  # any pointer may be NULL
        capi.check(plan._L.scn_plan_get_trace(plan.handle, 3, 5, None, None, only_count.ctypes.data_as(C.c_void_p)), "scn_plan_get_trace")
        assert np.array_equal(only_count, twice[2][3:8])
        # set_trace resets, also to another geometry; 0 cells drops the trace and the next one is empty again
        plan.set_trace(f0, cell_hz, cells)
        _check_trace(plan, trace_ref.new(cells), "reset")
        plan.set_trace(f0 + 5, cell_hz, cells + 9)
        plan.update_trace(0)
        _check_trace(plan, trace_ref.fold(trace_ref.new(cells + 9), f0 + 5, cell_hz, p, FS, centres[2]), "another geometry")
        plan.set_trace(0, 0, 0)
        assert _status(plan.update_trace, 0) == capi.E_STATE and _status(plan.trace, 0, 1) == capi.E_INVALID
        plan.set_trace(f0, cell_hz, 10)
        _check_trace(plan, trace_ref.new(10), "after a drop")


def test_fold_beside_a_pending_slot(built_lib):
    n, units = 1024, 4
    centres = _centres(units)
    xa, xb = synth.cfloat_batch(n, units, seed=31), synth.cfloat_batch(n, units, seed=32)
    kw = dict(threshold=2.0, max_batch=units)
    with Plan(n, FS, **kw) as solo:
        _submit(solo, 0, xb, center_freqs=centres)
        p_solo, h_solo, t_solo = solo.collect(0)
        assert len(h_solo) > 0
    with Plan(n, FS, **kw) as plan:
        plan.set_trace(97000000, 64 * (FS // n) + 7, 40)
        _submit(plan, 0, xa, center_freqs=centres)
        pa = plan.collect(0)[0]
        _submit(plan, 1, xb, center_freqs=centres)  # slot 1 stays pending
        assert _status(plan.update_trace, 1) == capi.E_STATE
        plan.update_trace(0)
        plan.set_trace(97000000, 64 * (FS // n) + 7, 40)  # allowed with a slot pending
        plan.update_trace(0)
        _check_trace(plan, trace_ref.fold(trace_ref.new(40), 97000000, 64 * (FS // n) + 7, pa, FS, centres), "beside a pending slot")
        pb, hb, tb = plan.collect(1)
        assert pb.tobytes() == p_solo.tobytes() and hb.tobytes() == h_solo.tobytes() and np.array_equal(tb, t_solo)


def test_state(built_lib):
    n, units = 16, 2
    centres = _centres(units)
    x = _noise(n, units, seed=40)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        assert _status(plan.update_trace, 0) == capi.E_STATE  # never collected (and no trace)
        _submit(plan, 0, x, center_freqs=centres)
        plan.collect(0)
        assert _status(plan.update_trace, 0) == capi.E_STATE and b"no trace" in plan._L.scn_last_error()  # a list, but no trace
        plan.set_trace(96000000, 100000, 200)
        assert _status(plan.update_trace, 1) == capi.E_STATE  # a trace, but slot 1 was never collected
        plan.update_trace(0)
        assert plan.trace()[2].sum() > 0
        _submit(plan, 0, x, center_freqs=centres)
        assert _status(plan.update_trace, 0) == capi.E_STATE  # pending
        plan.collect(0)
        plan.update_trace(0)
        plan.set_table(centres)
        assert _status(plan.update_trace, 0) == capi.E_STATE  # the table changed: the list is gone
        _submit(plan, 0, x, nb=0, center_freqs=centres[:0])
        plan.collect(0)
        before = plan.trace()
        plan.update_trace(0)  # a submit of zero units: SCN_OK, nothing folded
        assert trace_ref.same(plan.trace(), before)
        assert _status(plan.update_trace, capi.NUM_SLOTS) == capi.E_INVALID


def test_set_trace_refusals(built_lib):
    n = 16
    with Plan(n, FS, max_batch=1, **QUIET) as plan:
        assert _status(plan.set_trace, 0, 0, 8) == capi.E_INVALID
        assert _status(plan.set_trace, 0, 1, capi.TRACE_CELLS_MAX + 1) == capi.E_INVALID
        plan.set_trace(0, 1, capi.TRACE_CELLS_MAX)
        _check_trace(plan, trace_ref.new(capi.TRACE_CELLS_MAX), "the largest trace")
        plan.set_trace(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 1)
    refused = [dict(mode=capi.MODE_TIME_DOMAIN), dict(flags=capi.OUT_SPECTRUM), dict(flags=capi.OUT_HITS)]  # (fixed threshold, hits only)
    for kw in refused:
        with Plan(n, FS, max_batch=1, **QUIET, **kw) as plan:
            assert _status(plan.set_trace, 0, 1000, 8) == capi.E_INVALID, kw
            assert _status(plan.update_trace, 0) == capi.E_INVALID and _status(plan.trace, 0, 0) == capi.E_INVALID, kw
    for kw in (dict(detect=capi.DETECT_FLOOR, flags=capi.OUT_HITS), dict(detect=capi.DETECT_BASELINE, flags=capi.OUT_HITS, baseline=1)):
        with Plan(n, FS, max_batch=1, threshold=0.0, **kw) as plan:
            plan.set_trace(0, 1000, 8)


def test_units_outnumber_the_resident_teams(built_lib):
    """n = 16: a batch of twice the launcher's cap in units plus a small odd remainder takes every team through its loop twice and
    some a third time; six wide cells, so that every workgroup's atomics land on the same few words"""
    n = 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = trace_caps.trace_cap(cus, n)
    units = launch_caps.two_trips_and(cap, 5)
    assert launch_caps.trip_of(units - 1, cap) == 2
    rng = np.random.default_rng(50)
    centres = 100e6 + 250000.0 * rng.integers(0, 40, units)  # forty centres over 10 MHz, in no order
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _noise(n, units, seed=51), center_freqs=centres)
        p = plan.collect(0)[0]
        _fold_geometries(plan, 0, p, centres, "past the grid", geoms=[(96000000, 3000000, 6), (97000000, FS // n, 24), (96000000, 1, 1 << 22)])
