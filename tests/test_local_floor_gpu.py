"""The floor window on the GPU (scn_plan_set_floor_window, scn_floor_local.hip).  Every case runs a windowed floor plan with
SCN_OUT_SPECTRUM | SCN_OUT_HITS and asserts, with no bin exempt and no tolerance (an order statistic is exact):
  1. the full hit list equals tests/local_floor_ref.py's list from the plan's own returned spectrum: i, the bits of power_db,
     freq_hz, seq_id, the order, the trigger;
  2. the spectrum is byte-identical to that of a fixed SCN_OUT_SPECTRUM-only plan on the same input;
  3. a hits-only windowed plan on the same input returns the same records, byte for byte;
  4. capi.local_floor_from_spectrum on each unit gives the same cuts as the reference, bit for bit."""
import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi
from tests import floor_ref, local_floor_ref, signals_ref
from tests import tolerances as tol
from tests.test_floor_gpu import _straddling, _submit

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS


def _check(n, x, threshold, window, permille=0, kind=capi.KIND_FLOAT_COMPLEX, enob=12, average=1, layout=capi.AVG_DWELL, trigger_count=1047,
           indexed=False, want_parts=None, use_bandwidth=0.75, dc_ignore_bins=4):
    """the four assertions above on one input; returns (spectrum, hits, trigger) of the spectrum + hits plan"""
    nb = x.shape[0]
    units = nb // average
    train, guard = window
    mask = dict(use_bandwidth=use_bandwidth, dc_ignore_bins=dc_ignore_bins)  # every plan's, the reference's and the host form's
    kw = dict(kind=kind, enob=enob, max_batch=nb, average=average, average_layout=layout, trigger_count=trigger_count, **mask)
    fc_units = 100e6 + 6e6 * np.arange(units)
    if indexed:  # a run of the plan's table that wraps
        table = 100e6 + 6e6 * np.arange(units + 2)
        first = 3
        fc_units = table[(first + np.arange(units)) % table.size]
        sub = dict(first_index=first)
        seq_units = np.arange(units, dtype=np.uint64) * (average if layout == capi.AVG_DWELL else 1)
    else:
        members0 = np.arange(units) * average if layout == capi.AVG_DWELL else np.arange(units)  # each group's first buffer
        fc = np.empty(nb)
        for g in range(units):
            fc[(g * average + np.arange(average)) if layout == capi.AVG_DWELL else (g + units * np.arange(average))] = fc_units[g]
        seq = 1000 + 3 * np.arange(nb, dtype=np.uint64)
        seq_units = seq[members0]
        sub = dict(center_freqs=fc, seq_ids=seq)
    out = {}
    for flags in (BOTH, capi.OUT_HITS):
        with Plan(n, FS, threshold, flags=flags, detect=capi.DETECT_FLOOR, floor_permille=permille, floor_window=window, **kw) as plan:
            if indexed:
                plan.set_table(table)
            if want_parts is not None:
                assert (plan.average_parts(nb) > 1) == want_parts
            _submit(plan, 0, x, **sub)
            p, h, t = plan.collect(0)
            assert len(h) == plan.last_n_hits
            out[flags] = (p, h.copy(), t)
    p, h, t = out[BOTH]
    assert p.shape == (units, n)
    want_fl, want_h, want_t = local_floor_ref.detect(p, threshold, train, guard, permille, fc_units, seq_units, FS, trigger_count, **mask)
    floor_ref.assert_same_records(h, want_h, f"n {n} window {window}: the windowed plan against the reference")     # 1
    assert np.array_equal(t, want_t)
    with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, **kw) as plan:                                                    # 2
        _submit(plan, 0, x)
        p_fixed = plan.collect(0)[0]
    assert p_fixed.tobytes() == p.tobytes(), "the windowed plan's spectrum differs from the fixed spectrum-only plan's"
    p2, h2, t2 = out[capi.OUT_HITS]                                                                                  # 3
    assert p2 is None and h2.tobytes() == h.tobytes() and np.array_equal(t2, t)
    ev = tol.evaluated_mask(n, use_bandwidth, dc_ignore_bins)                                                        # 4
    for u in range(units):
        host = capi.local_floor_from_spectrum(p[u], train, guard, floor_permille=permille, **mask)
        assert floor_ref.same_bits(floor_ref.cut_of(host[ev], threshold), floor_ref.cut_of(want_fl[u][ev], threshold)), u
    return p, h, t


# (16, 5) under (1, 0): M_i is 1 or 2 everywhere; 64 x 3000: several units per workgroup, in many workgroups; 512: the largest
# wave-per-unit size; 1000: mixed radix; 1001: an odd n's rotation, Bluestein; 4096: a workgroup per unit, under the reference window
# and the largest one; 16384: the largest size staged in one piece; 65536: tiles, whose halos are the neighbouring tiles' bins
SHAPES = [(16, 5, (1, 0)), (64, 3000, (4, 1)), (512, 40, (16, 2)), (1000, 5, (16, 2)), (1001, 5, (16, 2)), (4096, 5, (16, 2)),
          (4096, 5, (128, 64)), (16384, 3, (128, 64)), (65536, 2, (128, 64))]


@pytest.mark.parametrize("n,nb,window", SHAPES)
def test_noise_straddling_0_db(built_lib, n, nb, window):
    p, h, t = _check(n, _straddling(n, nb, seed=n), 1.0, window, trigger_count=n // 4)
    band = p[:, tol.evaluated_mask(n)]
    assert band.min() < 0.0 < band.max(), "the in-band values do not straddle 0 dB"
    # 1.0 above the lower median of M cells, |X|^2 exponential: a hit with probability prod (k / (k + 10^0.2)) over k = M/2 + 1 ... M --
    # 0.41 at M = 8, 0.35 at 32, 0.34 at 256; fewer cells at the band's edges move it little.  (n = 16: 30 bins in all, M of 1 or 2)
    assert 0 < len(h) < band.size
    if n >= 64:
        assert band.size / 6 < len(h) < band.size / 2, (len(h), band.size)


# (n, teams per CU the launcher can make resident at the most, units beyond them): a wave per unit, 8 workgroups of 4 waves per CU;
# a 1024-thread workgroup per unit, 2 per CU (scn_floor_local.hip, launch)
@pytest.mark.parametrize("n,teams_per_cu,extra", [(64, 32, 1500), (8192, 2, 40)])
def test_units_outnumber_the_resident_teams(built_lib, n, teams_per_cu, extra):
    """The persistent loop: more units than the grid can hold teams, whatever the device's CU count, so that teams take a second
    unit -- with the first unit's cells in LDS, its count and its registers behind them.  Every unit is its own noise."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = cus * teams_per_cu + extra
    p, h, t = _check(n, _straddling(n, nb, seed=n + 1), 1.0, (4, 1), trigger_count=n // 4)
    assert len(np.unique(np.bincount(h["seq_id"].astype(np.int64)))) > 3


@pytest.mark.parametrize("permille", [capi.FLOOR_MIN, 1, 750, 1000])
def test_permille(built_lib, permille):
    n = 4096
    p, h, t = _check(n, _straddling(n, 5, seed=7), 0.5, (16, 2), permille)
    if permille == 1000:  # the floor is the window's maximum: a hit stands 0.5 above every one of its 32 cells
        assert 0 < len(h) < 0.05 * 5 * n
        ev = tol.evaluated_mask(n)
        fl = capi.local_floor_from_spectrum(p[0], 16, 2, floor_permille=1000)
        i = np.arange(n)
        by_i = np.where(ev, p[0], -np.inf)[(i + n // 2) % n]
        for c in (100 + 1000, 1800, 3000):  # interior bins: all 32 cells are evaluated
            cells = np.concatenate([by_i[c - 18:c - 2], by_i[c + 3:c + 19]])
            assert fl[(c + n // 2) % n] == cells.max()


@pytest.mark.parametrize("offset", [0.0, 3.0])
def test_int8_ties_and_minus_inf(built_lib, offset):
    """int8 input at ENOB 8: coarse samples (heavy ties), a constant buffer and an all-zero buffer, which has no hits"""
    n, nb = 4096, 5
    rng = np.random.default_rng(11)
    raw = rng.integers(-3, 4, (nb, n, 2)).astype(np.int8)
    raw[1] = 5
    raw[3] = 0
    p, h, t = _check(n, raw, offset, (16, 2), kind=capi.KIND_BYTE_COMPLEX, enob=8)
    assert np.all(np.isneginf(p[3]))
    assert not np.any(h["seq_id"] == 1000 + 3 * 3), "the all-zero unit reports hits"
    assert np.any(h["seq_id"] == 1000), "the noise unit reports nothing"


@pytest.mark.parametrize("layout", [capi.AVG_DWELL, capi.AVG_SWEEPS])
def test_averaged_units_are_groups(built_lib, layout):
    n, G, K = 1024, 3, 2
    _check(n, _straddling(n, G * K, seed=5), 0.5, (16, 2), average=K, layout=layout, trigger_count=100)


def test_averaged_split_route(built_lib):
    n, K = 1024, 16  # one group: its buffers are shared by several workgroups
    _check(n, _straddling(n, K, seed=6), 0.2, (16, 2), average=K, want_parts=True)


def test_indexed_submit(built_lib):
    _check(1024, _straddling(1024, 6, seed=8), 1.0, (16, 2), indexed=True)


def test_two_slots_in_flight(built_lib):
    """SCN_PLAN_OVERLAP_SLOTS: two submits pending on streams of their own, each collected with its own records"""
    n, nb = 4096, 6
    xs = [_straddling(n, nb, seed=20 + k) * np.float32(1.0 + 30.0 * k) for k in range(2)]
    with Plan(n, FS, 1.0, max_batch=nb, flags=BOTH | capi.PLAN_OVERLAP_SLOTS, detect=capi.DETECT_FLOOR, floor_window=(16, 2)) as plan:
        for rep in range(2):  # the second round reuses both slots (the other generation of regions and counts)
            for k in range(2):
                _submit(plan, k, xs[k ^ rep])
            for k in range(2):
                p, h, t = plan.collect(k)
                _, want_h, want_t = local_floor_ref.detect(p, 1.0, 16, 2, 0, None, None, FS)
                floor_ref.assert_same_records(h, want_h, f"round {rep} slot {k}")
                assert np.array_equal(t, want_t) and len(h) > nb
                assert np.array_equal(plan.hits_view(k), h[: len(plan.hits_view(k))])


@pytest.mark.parametrize("max_gap", [0, 7])
def test_signals_on_a_windowed_plan(built_lib, max_gap):
    n, nb = 4096, 4
    with Plan(n, FS, 2.0, max_batch=nb, detect=capi.DETECT_FLOOR, floor_window=(16, 2)) as plan:
        _submit(plan, 0, _straddling(n, nb, seed=9))
        h = plan.collect(0)[1]
        assert len(h) > nb
        got = plan.collect_signals(0, max_gap)
    signals_ref.assert_same(got, capi.signals_from_hits(h, n, FS, max_gap), f"max_gap {max_gap}: GPU against scn_signals_from_hits")
    assert int(got["n_hits"].sum()) == len(h)


def test_setter_states(built_lib):
    n, nb = 1024, 2
    x = _straddling(n, nb, seed=1)
    with Plan(n, FS, 0.0, max_batch=nb) as plan:  # a fixed plan has no floor to take from anywhere
        with pytest.raises(capi.ScannerError) as e:
            plan.set_floor_window(16, 2)
        assert e.value.status == capi.E_INVALID
    with pytest.raises(capi.ScannerError) as e:  # ... and the constructor's argument goes the same way
        Plan(n, FS, 0.0, max_batch=nb, floor_window=(16, 2))
    assert e.value.status == capi.E_INVALID
    with Plan(16, FS, 0.0, max_batch=nb, detect=capi.DETECT_FLOOR) as plan:  # the header's example
        plan.set_floor_window(1, 0)
        with pytest.raises(capi.ScannerError) as e:
            plan.set_floor_window(1, 1)
        assert e.value.status == capi.E_INVALID and "i = 3" in str(e.value)
    with Plan(n, FS, 1.0, max_batch=nb, detect=capi.DETECT_FLOOR) as plan:
        _submit(plan, 0, x)
        with pytest.raises(capi.ScannerError) as e:  # a slot is pending
            plan.set_floor_window(16, 2)
        assert e.value.status == capi.E_STATE
        p, h, t = plan.collect(0)
        want_fl, want_h, want_t = floor_ref.detect(p, 1.0, 0, None, None, FS)
        floor_ref.assert_same_records(h, want_h, "before any window: the unit-wide floor")
        assert floor_ref.same_bits(plan.collect_floor(0), want_fl)
        plan.set_floor_window(16, 2)
        assert floor_ref.same_bits(plan.collect_floor(0), want_fl)  # the collected slot keeps what it has
        for bad in ((0, 1), (129, 0), (1, 65)):  # refused, nothing changed: the window stays (16, 2)
            with pytest.raises(capi.ScannerError) as e:
                plan.set_floor_window(*bad)
            assert e.value.status == capi.E_INVALID
        _submit(plan, 0, x)
        p, h, t = plan.collect(0)
        floor_ref.assert_same_records(h, local_floor_ref.detect(p, 1.0, 16, 2, 0, None, None, FS)[1], "under the window (16, 2)")
        with pytest.raises(capi.ScannerError) as e:  # a windowed slot has no per-unit floor
            plan.collect_floor(0)
        assert e.value.status == capi.E_INVALID and "window" in str(e.value)
        plan.set_floor_window(0, 0)
        _submit(plan, 0, x)
        p, h, t = plan.collect(0)
        floor_ref.assert_same_records(h, want_h, "the window taken away: the unit-wide floor again")
        assert floor_ref.same_bits(plan.collect_floor(0), want_fl)


def _plateau_scene(n=4096, units=4, seed=42):
    """noise of sigma 0.01 per component; a plateau 20 dB of power above it over the bins i in [2600, 3300), synthesised in the
    frequency domain at 0.1 sqrt(n) per component; a tone of amplitude 0.2 on the plateau (i = 2950) and one of 0.003 in the quiet
    part (i = 1200), both on bin centres"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((units, n, 2)) * 0.01).view(np.complex128).reshape(units, n)
    X = np.zeros((units, n), np.complex128)
    j = (np.arange(2600, 3300) + n // 2) % n
    X[:, j] = (rng.standard_normal((units, j.size, 2)) * 0.1 * np.sqrt(n)).view(np.complex128).reshape(units, j.size)
    x += np.fft.ifft(X, axis=1)
    t = np.arange(n)
    for amp, i in ((0.2, 2950), (0.003, 1200)):
        x += amp * np.exp(2j * np.pi * ((i + n // 2) % n) * t / n)
    return x.astype(np.complex64), (2950, 1200)


def test_a_narrow_signal_on_a_wide_one(built_lib):
    """What the window is for.  Under the unit-wide floor the wide emitter is thousands of records and the tone on it is one hit among
    them; under a (16, 2) window the plateau is its own floor, and the tone on it and the weak one beside it are what is reported."""
    n, units, offset = 4096, 4, 6.0
    x, planted = _plateau_scene(n, units)
    hits = {}
    for window in (None, (16, 2)):
        with Plan(n, FS, offset, max_batch=units, detect=capi.DETECT_FLOOR, floor_window=window) as plan:
            _submit(plan, 0, x)
            hits[window] = plan.collect(0)[1]
    inner = np.arange(2640, 3260)
    inner = inner[np.abs(inner - planted[0]) > 4]  # 40 in from the plateau's edges, outside the tone's main lobe
    for u in range(units):
        wide = hits[None]["i"][hits[None]["seq_id"] == u]
        local = hits[(16, 2)]["i"][hits[(16, 2)]["seq_id"] == u]
        assert np.isin(inner, wide).sum() > 0.7 * inner.size, (u, np.isin(inner, wide).sum())
        assert np.isin(inner, local).sum() <= 3, (u, local[np.isin(local, inner)])
        assert planted[0] in local and planted[1] in local, (u, local)
