"""The floor detector on the GPU (scn_plan_desc.detect = SCN_DETECT_FLOOR, scn_floor.hip).  Every case runs a floor plan with
SCN_OUT_SPECTRUM | SCN_OUT_HITS and asserts, with no bin exempt and no tolerance (an order statistic is exact):
  1. collect_floor equals tests/floor_ref.py on the plan's own returned spectrum, and capi.floor_from_spectrum, bit for bit;
  2. the full hit list equals floor_ref's list from that spectrum: i, the bits of power_db, freq_hz, seq_id, the order, the trigger;
  3. the spectrum is byte-identical to that of a fixed SCN_OUT_SPECTRUM-only plan on the same input;
  4. a hits-only floor plan on the same input returns the same floors and the same records, byte for byte."""
import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi
from tests import floor_ref, signals_ref

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS


def _noise(n, nb, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nb, n, 2), dtype=np.float32) * np.float32(sigma)).view(np.complex64).reshape(nb, n)


def _straddling(n, nb, seed):
    """noise whose in-band dB values (10 log10 |X|) straddle 0: under the Blackman-Harris window (sum w^2 = 0.258 n) |X| is
    Rayleigh with rms sigma sqrt(2 * 0.258 n) and median 0.83 of that, which sigma = 1.67 / sqrt(n) puts at 1, i.e. 0 dB"""
    return _noise(n, nb, seed, sigma=1.67 / np.sqrt(n))


def _submit(plan, slot, x, nb=None, **kw):
    d_raw = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    plan.submit_device(slot, d_raw, x.shape[0] if nb is None else nb, **kw)


def _check(n, x, threshold, permille=0, kind=capi.KIND_FLOAT_COMPLEX, enob=12, average=1, layout=capi.AVG_DWELL, trigger_count=1047,
           indexed=False, want_parts=None, use_bandwidth=0.75, dc_ignore_bins=4):
    """the four assertions above on one input; returns (spectrum, floors, hits) of the spectrum + hits floor plan"""
    nb = x.shape[0]
    units = nb // average
    mask = dict(use_bandwidth=use_bandwidth, dc_ignore_bins=dc_ignore_bins)  # every plan's, the reference's and the host form's
    kw = dict(kind=kind, enob=enob, max_batch=nb, average=average, average_layout=layout, trigger_count=trigger_count, **mask)
    fc_units = 100e6 + 6e6 * np.arange(units)
    sub = {}
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
        with Plan(n, FS, threshold, flags=flags, detect=capi.DETECT_FLOOR, floor_permille=permille, **kw) as plan:
            if indexed:
                plan.set_table(table)
            if want_parts is not None:
                assert (plan.average_parts(nb) > 1) == want_parts
            _submit(plan, 0, x, **sub)
            p, h, t = plan.collect(0)
            assert len(h) == plan.last_n_hits
            out[flags] = (p, h.copy(), t, plan.collect_floor(0))
    p, h, t, fl = out[BOTH]
    assert p.shape == (units, n) and fl.shape == (units,)
    want_fl, want_h, want_t = floor_ref.detect(p, threshold, permille, fc_units, seq_units, FS, trigger_count, **mask)
    assert floor_ref.same_bits(fl, want_fl), (fl, want_fl)                                        # 1
    for u in range(units):
        assert floor_ref.same_bits(fl[u], capi.floor_from_spectrum(p[u], floor_permille=permille, **mask)), u
    floor_ref.assert_same_records(h, want_h, f"n {n}: the floor plan against the reference")      # 2
    assert np.array_equal(t, want_t)
    with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, **kw) as plan:                                  # 3
        _submit(plan, 0, x)
        p_fixed = plan.collect(0)[0]
    assert p_fixed.tobytes() == p.tobytes(), "the floor plan's spectrum differs from the fixed spectrum-only plan's"
    p2, h2, t2, fl2 = out[capi.OUT_HITS]                                                          # 4
    assert p2 is None and fl2.tobytes() == fl.tobytes() and h2.tobytes() == h.tobytes() and np.array_equal(t2, t)
    return p, fl, h


# 16: M is a handful of bins, ranks 0, (M - 1) / 2 and M - 1 all corner cases; 64 x 3000: several units per workgroup, in many
# workgroups (NOT the persistent loop: the grid still holds a team per unit -- test_units_outnumber_the_resident_teams is that
# case); 512: the largest wave-per-unit size; 1000: mixed radix; 1001: Bluestein; 4096, 8192: a workgroup per unit (256 and 1024
# threads); 16384: the largest size kept in registers; 65536: the route that re-reads
SHAPES = [(16, 5), (64, 3000), (512, 40), (1000, 5), (1001, 5), (4096, 5), (8192, 5), (16384, 3), (65536, 2)]


@pytest.mark.parametrize("offset", [0.0, 3.0])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_noise_straddling_0_db(built_lib, n, nb, offset):
    p, fl, h = _check(n, _straddling(n, nb, seed=n), offset, trigger_count=n // 8)
    from tests import tolerances as tol

    band = p[:, tol.evaluated_mask(n)]
    assert band.min() < 0.0 < band.max(), "the in-band values do not straddle 0 dB"
    if offset == 0.0:  # at the median: about half the evaluated bins, and so some units over the trigger count and (n = 16) some not
        assert 0.4 * band.size < len(h) < 0.6 * band.size, (len(h), band.size)
    else:
        assert (band.size < 1000 or 0 < len(h)) and len(h) < 0.3 * band.size, (len(h), band.size)  # (a Rayleigh tail of 1 / 16)


# (n, teams per CU the launcher can make resident at the most, units beyond them): a wave per unit, 8 workgroups of 4 waves per
# CU; a 256-thread workgroup per unit, 8 per CU; a 1024-thread workgroup per unit, 2 per CU (scn_floor.hip, launch)
@pytest.mark.parametrize("n,teams_per_cu,extra", [(64, 32, 1500), (1024, 8, 150), (8192, 2, 40)])
def test_units_outnumber_the_resident_teams(built_lib, n, teams_per_cu, extra):
    """The persistent loop: more units than the grid can hold teams, whatever the device's CU count, so that teams take a
    second unit -- with the first unit's histograms, its count and its registers behind them.  Every unit is its own noise, with
    its own floor and its own number of hits; all four assertions of _check, bit for bit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = cus * teams_per_cu + extra
    p, fl, h = _check(n, _straddling(n, nb, seed=n + 1), 1.0, trigger_count=n // 8)
    assert len(np.unique(fl)) > nb // 2 and len(np.unique(np.bincount(h["seq_id"].astype(np.int64)))) > 3


@pytest.mark.parametrize("permille", [capi.FLOOR_MIN, 1, 250, 999, 1000])
def test_permille(built_lib, permille):
    n = 4096
    p, fl, h = _check(n, _straddling(n, 5, seed=7), 0.5, permille)
    if permille == 1000:
        assert len(h) == 0  # nothing lies above the maximum
    if permille == capi.FLOOR_MIN:
        from tests import tolerances as tol

        assert np.array_equal(fl, p[:, tol.evaluated_mask(n)].min(axis=1))


@pytest.mark.parametrize("offset", [0.0, 3.0])
def test_int8_ties_and_minus_inf(built_lib, offset):
    """int8 input at ENOB 8: coarse samples (heavy ties), a constant buffer and an all-zero buffer, whose floor is -inf and which
    has no hits"""
    n, nb = 4096, 5
    rng = np.random.default_rng(11)
    raw = rng.integers(-3, 4, (nb, n, 2)).astype(np.int8)
    raw[1] = 5
    raw[3] = 0
    p, fl, h = _check(n, raw, offset, kind=capi.KIND_BYTE_COMPLEX, enob=8)
    assert np.all(np.isneginf(p[3])) and np.isneginf(fl[3])
    assert not np.any(h["seq_id"] == 1000 + 3 * 3), "the all-zero unit reports hits"
    assert np.any(h["seq_id"] == 1000), "the noise unit reports nothing"


@pytest.mark.parametrize("layout", [capi.AVG_DWELL, capi.AVG_SWEEPS])
def test_averaged_units_are_groups(built_lib, layout):
    n, G, K = 1024, 3, 2
    _check(n, _straddling(n, G * K, seed=5), 0.0, average=K, layout=layout, trigger_count=100)


def test_averaged_split_route(built_lib):
    n, K = 1024, 16  # one group: its buffers are shared by several workgroups
    _check(n, _straddling(n, K, seed=6), 0.0, average=K, want_parts=True)


def test_indexed_submit(built_lib):
    _check(1024, _straddling(1024, 6, seed=8), 0.0, indexed=True)


def test_two_slots_in_flight(built_lib):
    """SCN_PLAN_OVERLAP_SLOTS: two submits pending on streams of their own, each collected with its own floors and records"""
    n, nb = 4096, 6
    xs = [_straddling(n, nb, seed=20 + k) * np.float32(1.0 + 30.0 * k) for k in range(2)]
    with Plan(n, FS, 1.0, max_batch=nb, flags=BOTH | capi.PLAN_OVERLAP_SLOTS, detect=capi.DETECT_FLOOR) as plan:
        for rep in range(2):  # the second round reuses both slots (the other generation of regions and counts)
            for k in range(2):
                _submit(plan, k, xs[k ^ rep])
            for k in range(2):
                p, h, t = plan.collect(k)
                fl = plan.collect_floor(k)
                want_fl, want_h, want_t = floor_ref.detect(p, 1.0, 0, None, None, FS)
                assert floor_ref.same_bits(fl, want_fl)
                floor_ref.assert_same_records(h, want_h, f"round {rep} slot {k}")
                assert np.array_equal(t, want_t)
                assert np.array_equal(plan.hits_view(k), h[: len(plan.hits_view(k))])
        assert abs(float(np.median(plan.collect_floor(0))) - float(np.median(plan.collect_floor(1)))) > 10.0  # the two gains


@pytest.mark.parametrize("max_gap", [0, 7])
def test_signals_on_a_floor_plan(built_lib, max_gap):
    n, nb = 4096, 4
    with Plan(n, FS, 2.0, max_batch=nb, detect=capi.DETECT_FLOOR) as plan:
        _submit(plan, 0, _straddling(n, nb, seed=9))
        h = plan.collect(0)[1]
        assert len(h) > nb
        got = plan.collect_signals(0, max_gap)
    signals_ref.assert_same(got, capi.signals_from_hits(h, n, FS, max_gap), f"max_gap {max_gap}: GPU against scn_signals_from_hits")
    assert int(got["n_hits"].sum()) == len(h)


def test_collect_floor_state_and_mode(built_lib):
    n, nb = 1024, 2
    x = _straddling(n, nb, seed=1)
    with Plan(n, FS, 0.0, max_batch=nb) as plan:  # a fixed plan has no floors
        _submit(plan, 0, x)
        plan.collect(0)
        with pytest.raises(capi.ScannerError) as e:
            plan.collect_floor(0)
        assert e.value.status == capi.E_INVALID
    with Plan(n, FS, 0.0, max_batch=nb, detect=capi.DETECT_FLOOR) as plan:
        plan._nb[0] = nb
        with pytest.raises(capi.ScannerError) as e:  # never submitted
            plan.collect_floor(0)
        assert e.value.status == capi.E_STATE
        _submit(plan, 0, x)
        with pytest.raises(capi.ScannerError) as e:  # pending
            plan.collect_floor(0)
        assert e.value.status == capi.E_STATE
        plan.collect(0)
        assert plan.collect_floor(0).shape == (nb,)


def _tone_scene(n, units, gain):
    """noise of sigma 0.01 per component and a tone of amplitude 0.3 at natural bin 700 + 100 u + 0.37 (u mod 3), all in band"""
    x = _noise(n, units, seed=42, sigma=0.01).astype(np.complex64)
    t = np.arange(n)
    f = np.array([700 + 100 * u + 0.37 * (u % 3) for u in range(units)])
    for u in range(units):
        x[u] += (0.3 * np.exp(2j * np.pi * f[u] * t / n)).astype(np.complex64)
    return x * np.float32(gain), f


def test_the_threshold_rides_on_the_gain(built_lib):
    """What the mode is for: the same plan finds the same tone at two gains 60 dB of power apart, where a fixed threshold that is
    right at the first gain is blind at the second."""
    n, units, offset = 4096, 6, 10.0
    floors = {}
    for gain in (1.0, 2.0 ** -10):
        x, f = _tone_scene(n, units, gain)
        with Plan(n, FS, offset, max_batch=units, detect=capi.DETECT_FLOOR) as plan:
            _submit(plan, 0, x)
            p, h, t = plan.collect(0)
            floors[gain] = plan.collect_floor(0)
        for u in range(units):
            i_planted = (int(round(f[u])) + n // 2) % n
            hu = h["i"][h["seq_id"] == u].astype(np.int64)
            assert i_planted in hu, (gain, u, hu)
            assert np.all(np.abs(hu - i_planted) <= 4), (gain, u, hu)
            assert 3 <= hu.size <= 9, (gain, u, hu)
    assert np.all(floors[1.0] - floors[2.0 ** -10] > 29.0)  # 2^-10 in amplitude is 30.1 units of this dB scale
    fixed = float(floors[1.0][0]) + offset
    counts = {}
    for gain in (1.0, 2.0 ** -10):
        x, _ = _tone_scene(n, units, gain)
        with Plan(n, FS, fixed, max_batch=units) as plan:
            _submit(plan, 0, x)
            counts[gain] = len(plan.collect(0)[1])
    assert counts[1.0] > 0 and counts[2.0 ** -10] == 0, counts
