"""The level histogram on the GPU (scn_plan_set_levels, scn_plan_update_levels, scn_plan_get_levels, scn_plan_levels_summary;
scn_levels.hip).  Every assertion is an equality of integers: EVERY counter of every case, and every cell of every summary.
tests/levels_ref.py, the numpy model written from the definition, is fed the spectrum and the centres the plan itself returned: the
fold is a pure function of them (integers and compares only), so there is no tolerance and nothing exempt.
capi.levels_fold_spectrum, the host form, is held to the same integers beside it.

One submit per case, then one scn_plan_set_levels + scn_plan_update_levels per geometry and table (set_levels zeroes; a collected
slot may be folded any number of times).  The geometries are those of tests/test_trace_cpu.py; one whose cells times the table's
levels exceed SCN_LEVELS_WORDS_MAX keeps f0_hz and cell_hz and as many cells as that limit allows.  The tables are cut from the
spectrum itself: a value equal to an edge occurs in every one of them."""
import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi, synth
from tests import launch_caps, levels_caps, levels_ref, trace_ref
from tests.test_floor_gpu import _noise, _straddling, _submit
from tests.test_levels_cpu import clip, on_an_edge, own_values
from tests.test_trace_cpu import geometries
from tests.test_trace_gpu import _centres, _status

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS
QUIET = dict(threshold=1e9)  # a fixed threshold nothing exceeds: the histogram does not depend on the hits


def _edges(p, k):
    """k edges (float32, strictly increasing) across the finite values of the spectra p, several of them values of p itself"""
    own = own_values(p)
    assert own.size >= 4
    mid = float(np.floor(own[own.size // 2]))
    if k == 1:
        e = own[own.size // 2: own.size // 2 + 1]
    elif k == 7:
        e = np.concatenate([[-np.inf], own[np.linspace(0, own.size - 1, 7).astype(int)[1:-1]], [np.inf]]).astype(np.float32)
    elif k == 63:  # one unit apart around the middle; every eighth gives way to the value of p next above it
        e = (mid - 31 + np.arange(63)).astype(np.float32)
        for x in range(0, 63, 8):
            above = own[(own > e[x]) & (own < e[x] + 1)]
            if above.size:
                e[x] = above[0]
        e[31] = own[own.size // 2]  # (in [mid, mid + 1): between its neighbours)
    else:
        picked = np.unique(own[np.linspace(0, own.size - 1, min(own.size, 100)).astype(int)])
        rest = np.linspace(mid - 90.0, mid + 40.0, 400).astype(np.float32)
        rest = rest[~np.isin(rest, picked)]
        e = np.unique(np.concatenate([picked, rest[np.linspace(0, rest.size - 1, k - picked.size).astype(int)]]))
    assert e.size == k and levels_ref.edges_valid(e) and on_an_edge(p, e) > 0, k
    return e


def _check_levels(plan, want, what):
    got = plan.levels()
    assert levels_ref.same(got, want), (what, levels_ref.describe(got, want))
    return got


def _check_summary(plan, hist, what, queries=((0, 0), (500, 1), (1000, None))):
    """the summary kernel on the plan's histogram (== hist) against the model: all cells, and a window at each end"""
    cells, n_levels = hist.shape
    for permille, level in queries:
        level = n_levels - 1 if level is None else level
        want = levels_ref.summary(hist, permille, level)
        for first, count in ((0, cells), (0, min(3, cells)), (cells - min(5, cells), min(5, cells))):
            got = plan.levels_summary(permille, level, first, count)
            for name, g, w in zip(("rank_level", "above", "total"), got, want):
                assert levels_ref.same(g, w[first:first + count]), (what, permille, level, first, count, name)


def _fold_geometries(plan, slot, p, centres, what, tables=(7, 63), geoms=None, sample_rate=FS, summary_below=4096, **mask):
    """for each geometry and table: a fresh histogram, the slot folded once, every counter against the model and the host form (and
    the summary, where the histogram has fewer than summary_below cells: the model walks them in Python); returns the bins counted"""
    counted = 0
    for f0, cell_hz, cells in geoms or geometries(plan.n, centres):
        for k in tables:
            edges, cells_k = _edges(p, k), clip(cells, k)
            plan.set_levels(f0, cell_hz, cells_k, edges)
            if cells_k * (k + 1) <= 1 << 20:
                _check_levels(plan, levels_ref.new(cells_k, k), (what, "zeroed"))
            plan.update_levels(slot)
            want = levels_ref.fold(levels_ref.new(cells_k, k), f0, cell_hz, edges, p, sample_rate, centres, **mask)
            _check_levels(plan, want, (what, f0, cell_hz, cells_k, k))
            host = levels_ref.new(cells_k, k)
            capi.levels_fold_spectrum(host, f0, cell_hz, edges, p, sample_rate, centres, **mask)
            assert levels_ref.same(host, want), (what, "host form", cell_hz, k)
            if cells_k < summary_below:
                _check_summary(plan, want, (what, cell_hz, k), queries=((500, 1),))
            counted += int(want.sum())
    assert counted > 0, (what, "no geometry counted a bin")
    return counted


# team of 64 (a wave per unit, several units per workgroup): 16 and 512 by 16-byte loads (1 and 2 in flight), 18 by 4-byte loads (rows
# 8-byte aligned); team of 256: 1024 and 4096 by 16-byte loads (1 and 4 in flight), 1001 by 4-byte loads; team of 1024: 8192 and 65536
# by 16-byte loads (2 and 4 in flight), 4098 by 4-byte loads.  _centres: a fraction and a whole number of hertz alternate, so both
# of the kernel's ways to a cell run
@pytest.mark.parametrize("n,units", [(16, 7), (18, 5), (512, 6), (1001, 3), (1024, 5), (4096, 4), (4098, 3), (8192, 3), (65536, 2)])
def test_sizes_teams_and_load_forms(built_lib, n, units):
    centres = _centres(units)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _noise(n, units, seed=n), center_freqs=centres)
        p = plan.collect(0)[0]
        assert np.isfinite(p).all()
        _fold_geometries(plan, 0, p, centres, f"n {n}", summary_below=300)


@pytest.mark.parametrize("n", [16, 4096, 8192])
def test_the_tile(built_lib, n):
    """a grid where every cell of a unit fits the team's tile, one where most do not, one where a whole unit falls into one cell
    (the largest same-word contention) -- each checked to be what it says by tests/levels_caps.py"""
    units, bs = 4, FS // n
    centres = _centres(units)
    lo = int(centres[0] - FS / 2)
    ev = trace_ref.evaluated(n)
    span_bins = int(np.flatnonzero(ev)[-1] - np.flatnonzero(ev)[0]) + 1
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _noise(n, units, seed=n + 2), center_freqs=centres)
        p = plan.collect(0)[0]
        fits_hz = 64 * bs + 7 if n >= 4096 else bs  # (n = 16: 13 bins of a unit in 16 cells)
        assert span_bins * bs // fits_hz + 2 <= levels_caps.tile_cells(n, 63)
        _fold_geometries(plan, 0, p, centres, (n, "fits the tile"), tables=(63,), geoms=[(lo + 1000003, fits_hz, (units * 6000000) // fits_hz)])
        assert span_bins > 3 * levels_caps.tile_cells(n, 255)
        _fold_geometries(plan, 0, p, centres, (n, "beyond the tile"), tables=(255,), geoms=[(lo + 1000003, bs, min((units * 6000000) // bs, 1 << 16))])
        got = _fold_geometries(plan, 0, p, centres, (n, "one cell"), tables=(7, 255), geoms=[(lo, 3 * FS, 3)])
        assert got == 2 * units * int(ev.sum())


@pytest.mark.parametrize("n", [16, 1024, 8192])
def test_units_outnumber_the_resident_teams(built_lib, n):
    """a batch of twice the launcher's cap in units plus a small odd remainder takes every team through its loop twice and some a
    third time -- the case that finds a tile not zeroed between a team's units; wide cells, so that every workgroup's atomics land on
    the same few words, and cells of one bin_step"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = levels_caps.levels_cap(cus, n)
    units = launch_caps.two_trips_and(cap, 5)
    assert launch_caps.trip_of(units - 1, cap) == 2
    rng = np.random.default_rng(50 + n)
    centres = 100e6 + 250000.0 * rng.integers(0, 40, units)  # forty centres over 10 MHz, in no order
    x = np.tile(_noise(n, 64, seed=51 + n), ((units + 63) // 64, 1))[:units]
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, x, center_freqs=centres)
        p = plan.collect(0)[0]
        _fold_geometries(plan, 0, p, centres, "past the grid, wide", tables=(63,), geoms=[(96000000, 3000000, 6)])
        _fold_geometries(plan, 0, p, centres, "past the grid, bin_step", tables=(7,), geoms=[(97000000, FS // n, min(10000000 // (FS // n), 1 << 14))])


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
            assert trace_ref.bin_freqs(n, FS, centres[0])[0] == (1 << 64) - 3000000
            bs = FS // n
            _fold_geometries(plan, 0, p, centres, (n, scene, "wrapped"), geoms=[((1 << 64) - 3000000, bs, 3000000 // bs), (0, 64 * bs, 40)])


def test_special_values(built_lib):
    n, units = 64, 4
    centres = _centres(units)
    x = _noise(n, units, seed=12)
    x[1] = 0  # |X| = 0 everywhere: -inf in every bin, counted
    x[2, 5] = np.float32(np.nan) + 0j  # one NaN sample: the whole unit is NaN and counts nothing
    x[3] *= np.float32(1e31)  # |X|^2 overflows: +inf in every bin, counted
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, x, center_freqs=centres)
        p = plan.collect(0)[0]
        assert np.all(np.isneginf(p[1])) and np.all(np.isnan(p[2])) and np.all(np.isposinf(p[3])) and np.isfinite(p[0]).all()
        _fold_geometries(plan, 0, p, centres, "specials")
        m = int(trace_ref.evaluated(n).sum())
        for edges in ([-np.inf, 0.0, np.inf], [-1000.0, 1000.0]):  # +-inf as edges and beside finite ones
            plan.set_levels(0, 0xFFFFFFFF, 1, edges)
            plan.update_levels(0)
            got = plan.levels()
            want = levels_ref.fold(levels_ref.new(1, len(edges)), 0, 0xFFFFFFFF, edges, p, FS, centres)
            assert levels_ref.same(got, want) and int(got.sum()) == 3 * m and got[0, -1] == m
            assert got[0, 0] == (0 if np.isinf(edges[0]) else m)  # (nothing is below -inf: -inf belongs to the level above that edge)
        plan.set_levels(int(centres[2] - FS / 2 + 2000000), 2000000, 1, [0.0])  # cells that only the NaN unit reaches
        plan.update_levels(0)
        assert int(plan.levels().sum()) == 0
        assert plan.levels_summary()[0].tolist() == [capi.LEVELS_NO_RANK]


def test_int16_input_with_dc_removal(built_lib):
    n, units = 1024, 5
    centres = _centres(units)
    raw = synth.quantize(synth.cfloat_batch(n, units, seed=3), capi.KIND_SHORT_COMPLEX)
    with Plan(n, FS, kind=capi.KIND_SHORT_COMPLEX, enob=12, correct_dc=True, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, raw, nb=units, center_freqs=centres)
        _fold_geometries(plan, 0, plan.collect(0)[0], centres, "int16")


def test_mask_of_the_plan(built_lib):
    n, units = 64, 3
    centres = _centres(units)
    for mask in (dict(dc_ignore_bins=0), dict(dc_ignore_bins=9, use_bandwidth=0.5), dict(use_bandwidth=1.0, dc_ignore_bins=1)):
        with Plan(n, FS, max_batch=units, **QUIET, **mask) as plan:
            _submit(plan, 0, _noise(n, units, seed=4), center_freqs=centres)
            _fold_geometries(plan, 0, plan.collect(0)[0], centres, mask, **mask)


def test_averaged_plan(built_lib):
    n, k, groups = 1024, 4, 3
    centres = _centres(groups)
    with Plan(n, FS, max_batch=k * groups, average=k, average_layout=capi.AVG_DWELL, **QUIET) as plan:
        _submit(plan, 0, _noise(n, k * groups, seed=6), center_freqs=np.repeat(centres, k))
        p = plan.collect(0)[0]
        assert p.shape == (groups, n)
        _fold_geometries(plan, 0, p, centres, "averaged")


@pytest.mark.parametrize("detect", [capi.DETECT_FLOOR, capi.DETECT_BASELINE])
def test_hits_only_detector_plans_against_their_twins(built_lib, detect):
    """a floor / baseline plan flagged hits-only keeps the spectrum its detect kernel reads in a buffer of its own: the histogram
    folded from it must be that of the SPECTRUM|HITS twin on the same input -- both run the spectrum-only transform.  That the two
    spectra are the same bits is not assumed here for the first time: the same kernel instantiation writes both, only its
    destination differs (the caller's buffer, or the plan's d_detect_power), and tests/test_trace_gpu.py holds the trace of the two
    routes to each other in the same way.  The twin itself is held to the model, so a difference here is the hits-only route's."""
    n, units = 4096, 4
    centres = _centres(units)
    x = _straddling(n, units, seed=n + 7)
    kw = dict(threshold=0.0, detect=detect, max_batch=units)
    if detect == capi.DETECT_BASELINE:
        kw["baseline"] = units
    hists, tables = {}, []
    for flags in (BOTH, capi.OUT_HITS):
        with Plan(n, FS, flags=flags, **kw) as plan:
            _submit(plan, 0, x, center_freqs=centres)
            p = plan.collect(0)[0]
            if flags == BOTH:
                tables = [_edges(p, 7), _edges(p, 63)]
                _fold_geometries(plan, 0, p, centres, (detect, "twin"))
            hists[flags] = []
            for f0, cell_hz, cells in geometries(n, centres):
                for edges in tables:
                    plan.set_levels(f0, cell_hz, clip(cells, edges.size), edges)
                    plan.update_levels(0)
                    hists[flags].append(plan.levels())
    assert len(hists[BOTH]) == len(hists[capi.OUT_HITS]) > 0
    for a, b in zip(hists[BOTH], hists[capi.OUT_HITS]):
        assert levels_ref.same(b, a) and int(a.sum()) > 0, (detect, levels_ref.describe(b, a))


def test_spectrum_in_the_callers_buffer_offset_by_four_bytes(built_lib):
    """n % 4 == 0, but the rows begin 4 bytes off a 16-byte boundary: the 4-byte loads"""
    n, units = 1024, 4
    centres = _centres(units)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        whole = torch.full((units * n + 4,), float("nan"), dtype=torch.float32, device="cuda")
        d_power = whole[1:1 + units * n]
        assert d_power.data_ptr() % 16 == 4
        _submit(plan, 0, _noise(n, units, seed=9), center_freqs=centres, d_power_db=d_power)
        plan.collect(0, want_power=False)
        torch.cuda.synchronize()
        p = d_power.cpu().numpy().reshape(units, n)
        assert np.isfinite(p).all()
        _fold_geometries(plan, 0, p, centres, "d_power_db + 4")


def test_against_the_trace(built_lib):
    """the trace and the histogram on one grid, one slot folded into both: the levels of a cell sum to the trace's count"""
    n, units = 1024, 5
    centres = _centres(units, step=5e6)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _noise(n, units, seed=13), center_freqs=centres)
        p = plan.collect(0)[0]
        for f0, cell_hz, cells in geometries(n, centres):
            cells = clip(cells, 63)
            plan.set_trace(f0, cell_hz, cells)
            plan.set_levels(f0, cell_hz, cells, _edges(p, 63))
            plan.update_trace(0)
            plan.update_levels(0)
            plan.update_levels(0)
            count = plan.trace()[2]
            assert count.sum() > 0 and np.array_equal(plan.levels().sum(axis=1, dtype=np.uint64), 2 * count)
            assert np.array_equal(plan.levels_summary()[2], 2 * count)


@pytest.mark.parametrize("k", [1, 63, 255])
def test_summary_kernel(built_lib, k):
    """one and four rounds of the scan; permille in {0, 500, 1000}, level in {0, 1, n_edges}, windows at both ends; empty cells, and
    cells folded eight times"""
    n, units = 4096, 4
    centres = _centres(units)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        _submit(plan, 0, _straddling(n, units, seed=14), center_freqs=centres)
        p = plan.collect(0)[0]
        edges = _edges(p, k)
        for f0, cell_hz, cells in ((int(centres[0]) - 6000000, 64 * (FS // n) + 7, 250), (int(centres[0]), 3 * FS, 2), (int(centres[1]), FS // n, 700)):
            plan.set_levels(f0, cell_hz, cells, edges)
            _check_summary(plan, levels_ref.new(cells, k), ("empty", k, cell_hz), queries=((500, 0),))
            want = levels_ref.new(cells, k)
            for _ in range(8):
                plan.update_levels(0)
                want = levels_ref.fold(want, f0, cell_hz, edges, p, FS, centres)
            _check_levels(plan, want, ("eight folds", k, cell_hz))
            assert (want.sum(axis=1) == 0).any() or cells == 2
            _check_summary(plan, want, (k, cell_hz), queries=[(pm, lv) for pm in (0, 500, 1000) for lv in (0, 1, None)])
            host = capi.levels_summary(want, 500, 1)
            assert all(levels_ref.same(g, w) for g, w in zip(plan.levels_summary(500, 1), host))
        for bad in (dict(permille=1001), dict(level=k + 1), dict(first=0, cells=701), dict(first=700, cells=1), dict(first=0xFFFFFFFF, cells=2)):
            assert _status(plan.levels_summary, **bad) == capi.E_INVALID, bad
        assert all(a.size == 0 for a in plan.levels_summary(first=700, cells=0))


def test_accumulation_reset_order_and_windows(built_lib):
    n, units = 512, 4
    centres = [_centres(units), _centres(units, first=103e6)]
    f0, cell_hz, cells = 97000000, 40 * (FS // n) + 3, 60
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        ps = []
        for slot in (0, 1):
            _submit(plan, slot, _noise(n, units, seed=20 + slot), center_freqs=centres[slot])
            ps.append(plan.collect(slot)[0])
        edges = _edges(np.concatenate(ps), 63)
        each = [levels_ref.fold(levels_ref.new(cells, 63), f0, cell_hz, edges, ps[s], FS, centres[s]) for s in (0, 1)]
        assert each[0].sum() > 0 and each[1].sum() > 0 and not levels_ref.same(each[0], each[1])
        for order in ((0, 1), (1, 0)):  # two slots folded in either order: the same integers
            plan.set_levels(f0, cell_hz, cells, edges)
            for slot in order:
                plan.update_levels(slot)
            _check_levels(plan, each[0] + each[1], ("order", order))
        plan.update_levels(0)
        plan.update_levels(1)  # every slot folded twice: every counter doubles
        twice = _check_levels(plan, 2 * (each[0] + each[1]), "folded twice")
        for first, count in ((0, cells), (7, 13), (cells - 1, 1), (cells, 0), (0, 0)):
            assert levels_ref.same(plan.levels(first, count), twice[first:first + count]), (first, count)
        for first, count in ((0, cells + 1), (cells, 1), (cells + 1, 0), (0xFFFFFFFF, 2)):
            assert _status(plan.levels, first, count) == capi.E_INVALID, (first, count)
        # set_levels zeroes, also to another geometry and table; 0 cells drops the histogram and the next one is empty again
        plan.set_levels(f0, cell_hz, cells, edges)
        _check_levels(plan, levels_ref.new(cells, 63), "reset")
        e7 = _edges(ps[0], 7)
        plan.set_levels(f0 + 5, cell_hz, cells + 9, e7)
        plan.update_levels(0)
        _check_levels(plan, levels_ref.fold(levels_ref.new(cells + 9, 7), f0 + 5, cell_hz, e7, ps[0], FS, centres[0]), "another geometry")
        plan.set_levels(0, 0, 0, e7)
        assert _status(plan.update_levels, 0) == capi.E_STATE and _status(plan.levels, 0, 1) == capi.E_INVALID
        plan.set_levels(f0, cell_hz, 10, e7)
        _check_levels(plan, levels_ref.new(10, 7), "after a drop")


def test_fold_beside_a_pending_slot(built_lib):
    n, units = 1024, 4
    centres = _centres(units)
    xa, xb = synth.cfloat_batch(n, units, seed=31), synth.cfloat_batch(n, units, seed=32)
    kw = dict(threshold=2.0, max_batch=units)
    geom = (97000000, 64 * (FS // n) + 7, 40)
    with Plan(n, FS, **kw) as solo:
        _submit(solo, 0, xb, center_freqs=centres)
        p_solo, h_solo, t_solo = solo.collect(0)
        assert len(h_solo) > 0
    with Plan(n, FS, **kw) as plan:
        _submit(plan, 0, xa, center_freqs=centres)
        pa = plan.collect(0)[0]
        edges = _edges(pa, 63)
        _submit(plan, 1, xb, center_freqs=centres)  # slot 1 stays pending
        plan.set_levels(*geom, edges)  # allowed with a slot pending
        assert _status(plan.update_levels, 1) == capi.E_STATE
        plan.update_levels(0)
        want = levels_ref.fold(levels_ref.new(40, 63), *geom[:2], edges, pa, FS, centres)
        _check_levels(plan, want, "beside a pending slot")
        _check_summary(plan, want, "beside a pending slot")
        pb, hb, tb = plan.collect(1)
        assert pb.tobytes() == p_solo.tobytes() and hb.tobytes() == h_solo.tobytes() and np.array_equal(tb, t_solo)


def test_state_refusals_are_the_traces(built_lib):
    """every refusal of scn_plan_update_trace, with the same status: both are asked at every step"""
    n, units = 16, 2
    centres = _centres(units)
    x = _noise(n, units, seed=40)
    edges = [-20.0, -10.0, 0.0]

    def both(plan, slot):
        a, b = _status(plan.update_trace, slot), _status(plan.update_levels, slot)
        assert a == b, (a, b)
        return b

    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        assert both(plan, 0) == capi.E_STATE  # never collected (and nothing to fold into)
        _submit(plan, 0, x, center_freqs=centres)
        plan.collect(0)
        assert both(plan, 0) == capi.E_STATE and b"no level histogram" in plan._L.scn_last_error()  # a list, but no histogram
        plan.set_trace(96000000, 100000, 200)
        plan.set_levels(96000000, 100000, 200, edges)
        assert both(plan, 1) == capi.E_STATE  # slot 1 was never collected
        assert both(plan, 0) == capi.OK
        assert plan.levels().sum() > 0
        _submit(plan, 0, x, center_freqs=centres)
        assert both(plan, 0) == capi.E_STATE  # pending
        plan.collect(0)
        assert both(plan, 0) == capi.OK
        plan.set_table(centres)
        assert both(plan, 0) == capi.E_STATE  # the table changed: the list is gone
        _submit(plan, 0, x, nb=0, center_freqs=centres[:0])
        plan.collect(0)
        before = plan.levels()
        assert both(plan, 0) == capi.OK  # a submit of zero units: SCN_OK, nothing folded
        assert levels_ref.same(plan.levels(), before)
        assert both(plan, capi.NUM_SLOTS) == capi.E_INVALID and both(plan, -1) == capi.E_INVALID


def test_set_levels_refusals(built_lib):
    n = 16
    good = [-1.0, 0.0, 1.0]
    with Plan(n, FS, max_batch=1, **QUIET) as plan:
        plan.set_levels(0, 1000000, 8, good)  # (the unit's evaluated bins lie at 1.0 ... 2.0 and 6.0 ... 7.0 MHz)
        _submit(plan, 0, _noise(n, 1, seed=41), center_freqs=[4e6])
        plan.collect(0)
        plan.update_levels(0)
        kept = plan.levels()
        assert kept.sum() > 0
        for bad in ((0, 0, 8, good), (0, 1, capi.TRACE_CELLS_MAX + 1, good), (0, 1, capi.LEVELS_WORDS_MAX // 4 + 1, good), (0, 1, 8, []),
                    (0, 1, 8, np.arange(256)), (0, 1, 8, [0.0, 0.0]), (0, 1, 8, [1.0, 0.0]), (0, 1, 8, [0.0, -0.0]), (0, 1, 8, [0.0, np.nan])):
            assert _status(plan.set_levels, *bad) == capi.E_INVALID, bad
            assert levels_ref.same(plan.levels(0, 8), kept), ("a refused set_levels changed the histogram", bad)
        assert plan._L.scn_plan_set_levels(plan.handle, 0, 1, 8, None, 3) == capi.E_INVALID
        plan.set_levels(0, 1, capi.LEVELS_WORDS_MAX // 4, good)  # the largest histogram
        assert plan.levels_summary(first=capi.LEVELS_WORDS_MAX // 4 - 2)[2].tolist() == [0, 0]
        plan.set_levels(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 1, np.arange(255))
    refused = [dict(mode=capi.MODE_TIME_DOMAIN), dict(flags=capi.OUT_SPECTRUM), dict(flags=capi.OUT_HITS)]  # (fixed threshold, hits only)
    for kw in refused:
        with Plan(n, FS, max_batch=1, **QUIET, **kw) as plan:
            assert _status(plan.set_levels, 0, 1000, 8, good) == capi.E_INVALID and _status(plan.set_trace, 0, 1000, 8) == capi.E_INVALID, kw
            assert _status(plan.update_levels, 0) == capi.E_INVALID and _status(plan.levels, 0, 0) == capi.E_INVALID, kw
            assert _status(plan.levels_summary, 500, 0, 0, 0) == capi.E_INVALID, kw
    for kw in (dict(detect=capi.DETECT_FLOOR, flags=capi.OUT_HITS), dict(detect=capi.DETECT_BASELINE, flags=capi.OUT_HITS, baseline=1)):
        with Plan(n, FS, max_batch=1, threshold=0.0, **kw) as plan:
            plan.set_levels(0, 1000, 8, good)
