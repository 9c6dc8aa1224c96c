"""The baseline detector on the GPU (scn_plan_desc.detect = SCN_DETECT_BASELINE, scn_baseline.hip).  Everything is an equality, with
no bin exempt and no tolerance -- the decision is one float addition and a compare, the update a copy or a compare of bits:
  1. the full hit list equals tests/baseline_ref.py's list from the plan's own returned spectrum: i, the bits of power_db, freq_hz,
     seq_id, the order, the trigger;
  2. the spectrum is byte-identical to that of a fixed SCN_OUT_SPECTRUM-only plan on the same input;
  3. a hits-only baseline plan on the same input returns the same records, byte for byte;
  4. the baseline after scn_plan_update_baseline equals baseline_ref.update, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi
from tests import baseline_ref, signals_ref
from tests import tolerances as tol
from tests.test_floor_gpu import _straddling, _submit

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS


@functools.lru_cache(maxsize=None)
def _spectrum(n, nb, seed, average=1, layout=capi.AVG_DWELL):
    """(input, its spectrum from a fixed spectrum-only plan): computed once per scene, shared and never written"""
    x = _straddling(n, nb, seed)
    with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, max_batch=nb, average=average, average_layout=layout) as plan:
        _submit(plan, 0, x)
        p = plan.collect(0)[0]
    p.setflags(write=False)
    return x, p


def _headers(nb, average, layout):
    """(submit keywords, fc per unit, seq per unit) of a plain submit, as tests/test_floor_gpu.py names its buffers"""
    units = nb // average
    fc_units = 100e6 + 6e6 * np.arange(units)
    fc = np.empty(nb)
    for g in range(units):
        fc[(g * average + np.arange(average)) if layout == capi.AVG_DWELL else (g + units * np.arange(average))] = fc_units[g]
    seq = 1000 + 3 * np.arange(nb, dtype=np.uint64)
    members0 = np.arange(units) * average if layout == capi.AVG_DWELL else np.arange(units)  # each group's first buffer
    return dict(center_freqs=fc, seq_ids=seq), fc_units, seq[members0]


def _check(n, x, baseline, threshold, want_spectrum=None, average=1, layout=capi.AVG_DWELL, trigger_count=1047, want_parts=None,
           flags_extra=0, use_bandwidth=0.75, dc_ignore_bins=4):
    """assertions 1 to 3 on one input against one baseline (a plain submit: unit u reads row u % rows); returns (spectrum, hits)"""
    nb = x.shape[0]
    units = nb // average
    sub, fc_units, seq_units = _headers(nb, average, layout)
    mask = dict(use_bandwidth=use_bandwidth, dc_ignore_bins=dc_ignore_bins)  # every plan's and the reference's
    out = {}
    for flags in (BOTH, capi.OUT_HITS):
        with Plan(n, FS, threshold, flags=flags | flags_extra, detect=capi.DETECT_BASELINE, baseline=baseline, max_batch=nb, average=average,
                  average_layout=layout, trigger_count=trigger_count, **mask) as plan:
            if want_parts is not None:
                assert (plan.average_parts(nb) > 1) == want_parts
            _submit(plan, 0, x, **sub)
            p, h, t = plan.collect(0)
            assert len(h) == plan.last_n_hits
            out[flags] = (p, h.copy(), t)
    p, h, t = out[BOTH]
    assert p.shape == (units, n)
    want_h, want_t = baseline_ref.detect(p, baseline, 0, threshold, fc_units, seq_units, FS, trigger_count, **mask)
    baseline_ref.assert_same_records(h, want_h, f"n {n}: the baseline plan against the reference")              # 1
    assert np.array_equal(t, want_t)
    if want_spectrum is not None:                                                                                # 2
        assert want_spectrum.tobytes() == p.tobytes(), "the baseline plan's spectrum differs from the fixed spectrum-only plan's"
    p2, h2, t2 = out[capi.OUT_HITS]                                                                              # 3
    assert p2 is None and h2.tobytes() == h.tobytes() and np.array_equal(t2, t)
    return p, h


# floor's list -- 16: a handful of evaluated bins; 64 x 3000: several units per workgroup, in many workgroups; 512: the largest
# wave-per-unit size, two loads in flight; 1000: mixed radix; 1001: Bluestein, an odd n: the 4-byte loads, row u 4-byte aligned only;
# 4096, 8192: a workgroup per unit (256 and 1024 threads); 16384: four loads in flight; 65536: the four-step pair, a loop of four
# trips -- plus 18: rows that are 8-byte but not 16-byte aligned, so the 4-byte loads at an even n
SHAPES = [(16, 5), (64, 3000), (512, 40), (1000, 5), (1001, 5), (4096, 5), (8192, 5), (16384, 3), (65536, 2), (18, 9)]


@pytest.mark.parametrize("threshold", [0.0, 3.0])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_noise_against_an_independent_draw(built_lib, n, nb, threshold):
    x, p_fixed = _spectrum(n, nb, seed=n)
    _, baseline = _spectrum(n, nb, seed=n + 100000)  # a row per unit
    p, h = _check(n, x, baseline, threshold, want_spectrum=p_fixed, trigger_count=n // 8)
    evaluated = nb * int(tol.evaluated_mask(n).sum())
    if threshold == 0.0 and evaluated >= 1000:  # two independent draws: a symmetric comparison
        assert 0.4 * evaluated < len(h) < 0.6 * evaluated, (len(h), evaluated)


def _lower(a):
    return np.nextafter(a, np.float32(-np.inf), dtype=np.float32)


@pytest.mark.parametrize("n", [64, 1001, 4096])
def test_the_compare_is_strict(built_lib, n):
    """against its own spectrum nothing is a hit; one ulp below it, exactly the lowered evaluated bins are"""
    units = 3
    x, p_fixed = _spectrum(n, units, seed=n + 7)
    p, h = _check(n, x, p_fixed, 0.0, want_spectrum=p_fixed)
    assert len(h) == 0
    ev = tol.evaluated_mask(n)
    i_ev = np.flatnonzero(ev[(np.arange(n) + n // 2) % n])  # the evaluated fftshift indices, increasing
    hole = n - n // 2  # the i of natural bin 0 (the middle of the DC hole)
    chosen_i = np.array([i_ev[0], i_ev[-1], i_ev[i_ev < hole].max(), i_ev[i_ev > hole].min(), i_ev[5], i_ev[-7]])
    masked_i = np.array([0, n - 1, i_ev[0] - 1, i_ev[-1] + 1, hole, hole - 1, hole + 2])  # out of band on both sides, inside the DC hole
    to_j = lambda i: (np.asarray(i) + n // 2) % n  # noqa: E731
    assert ev[to_j(chosen_i)].all() and not ev[to_j(masked_i)].any() and len(set(chosen_i)) == chosen_i.size
    assert {to_j(hole - 4), to_j(hole + 4)} <= set(to_j(chosen_i))  # both neighbours of the hole: natural bins n - 4 and 4
    baseline = p_fixed.copy()
    per_unit = [chosen_i, chosen_i[:2], chosen_i[:0]]  # unit 2: masked bins only
    for u in range(units):
        for i in np.concatenate([per_unit[u], masked_i]):
            baseline[u, to_j(i)] = _lower(baseline[u, to_j(i)])
    p, h = _check(n, x, baseline, 0.0, want_spectrum=p_fixed)
    seq = 1000 + 3 * np.arange(units)
    for u in range(units):
        assert np.array_equal(h["i"][h["seq_id"] == seq[u]], np.sort(per_unit[u])), u
    assert len(h) == chosen_i.size + 2


def test_rows_follow_the_table_and_wrap(built_lib):
    """the same noise in every unit against rows of constant, distinct levels: a unit's count tells which row it read"""
    n, units = 1024, 6
    x1, p1 = _spectrum(n, 1, seed=31)
    x = np.repeat(x1, units, axis=0)
    ev = tol.evaluated_mask(n)
    for rows, first in ((units + 2, 3), (1, 3)):
        table = 100e6 + 6e6 * np.arange(units + 2)
        levels = np.linspace(-4.0, 4.0, rows).astype(np.float32)
        baseline = np.repeat(levels[:, None], n, axis=1)
        with Plan(n, FS, 0.0, max_batch=units, detect=capi.DETECT_BASELINE, baseline=baseline, trigger_count=n // 8) as plan:
            plan.set_table(table)
            _submit(plan, 0, x, first_index=first)
            p, h, t = plan.collect(0)
        assert p.tobytes() == np.repeat(p1, units, axis=0).tobytes()
        row = (first + np.arange(units)) % rows
        want_h, want_t = baseline_ref.detect(p, baseline, first, 0.0, table[(first + np.arange(units)) % table.size], None, FS, n // 8)
        baseline_ref.assert_same_records(h, want_h, f"rows {rows}")
        assert np.array_equal(t, want_t)
        counts = np.bincount(h["seq_id"].astype(np.int64), minlength=units)
        assert np.array_equal(counts, [(p1[0][ev] > levels[r]).sum() for r in row])
        if rows > 1:  # rows 3 4 5 6 7 0: falling counts, then the lowest level's, the largest
            assert np.all(np.diff(counts[:5]) < 0) and counts[5] > counts[0] and len(set(counts)) == units


@pytest.mark.parametrize("rows", [1, 3])
def test_plain_submits_read_rows_from_zero(built_lib, rows):
    n, units = 1024, 7
    x, p_fixed = _spectrum(n, units, seed=32)
    baseline = np.repeat(np.linspace(-2.0, 2.0, rows).astype(np.float32)[:, None], n, axis=1)
    p, h = _check(n, x, baseline, 0.5, want_spectrum=p_fixed)
    assert len(h) > 0


# (n, teams per CU the launcher can make resident at the most, an odd rest beyond them): a wave per unit, 8 workgroups of 4 waves per
# CU; a 256-thread workgroup per unit, 8 per CU; a 1024-thread workgroup per unit, 2 per CU (scn_baseline.hip, launch)
@pytest.mark.parametrize("n,teams_per_cu,extra", [(64, 32, 1501), (1024, 8, 151), (8192, 2, 41)])
def test_units_outnumber_the_resident_teams(built_lib, n, teams_per_cu, extra):
    """The persistent loop: more units than the grid can hold teams, whatever the device's CU count, so that teams take a second
    unit -- with the first unit's count behind them.  Every unit is its own noise against a row of its own."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = cus * teams_per_cu + extra
    x, p_fixed = _spectrum(n, nb, seed=n + 1)
    _, baseline = _spectrum(n, nb, seed=n + 2)
    p, h = _check(n, x, baseline, 1.0, want_spectrum=p_fixed, trigger_count=n // 8)
    assert len(np.unique(np.bincount(h["seq_id"].astype(np.int64)))) > 3


@pytest.mark.parametrize("n,G,K,layout,parts", [(1024, 3, 2, capi.AVG_DWELL, None), (1024, 3, 2, capi.AVG_SWEEPS, None),
                                                (4096, 2, 16, capi.AVG_DWELL, True), (8192, 3, 2, capi.AVG_DWELL, None)])
def test_averaged_units_are_groups(built_lib, n, G, K, layout, parts):
    """K = 2 in both layouts; the split route, K = 16 over few groups (several workgroups share a group); the all-float 8192-point
    kernel.  The baseline has a row per GROUP, an averaged spectrum of an independent draw."""
    x, p_fixed = _spectrum(n, G * K, seed=n + 5, average=K, layout=layout)
    _, baseline = _spectrum(n, G * K, seed=n + 6, average=K, layout=layout)
    assert baseline.shape == (G, n)
    p, h = _check(n, x, baseline, 0.0, want_spectrum=p_fixed, average=K, layout=layout, trigger_count=100, want_parts=parts)
    assert 0 < len(h)


def test_special_values(built_lib):
    n, units = 4096, 4
    x = np.array(_spectrum(n, units, seed=41)[0])
    x[2] = 0  # an all-zero buffer: its spectrum is -inf
    with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, max_batch=units) as plan:
        _submit(plan, 0, x)
        p_fixed = plan.collect(0)[0]
    assert np.all(np.isneginf(p_fixed[2])) and np.all(np.isfinite(p_fixed[[0, 1, 3]]))
    ev_j = np.flatnonzero(tol.evaluated_mask(n))
    rng = np.random.default_rng(5)
    pick = rng.permutation(ev_j)
    j_inf, j_ninf, j_nan = pick[:40], pick[40:80], pick[80:120]
    baseline = np.array(_spectrum(n, units, seed=42)[1])
    baseline[:, j_inf], baseline[:, j_ninf], baseline[:, j_nan] = np.inf, -np.inf, np.nan
    p, h = _check(n, x, baseline, 0.0, want_spectrum=p_fixed)
    seq = 1000 + 3 * np.arange(units)
    to_i = lambda j: (np.asarray(j) + n - n // 2) % n  # noqa: E731
    for u in (0, 1, 3):
        hu = set(h["i"][h["seq_id"] == seq[u]])
        assert set(to_i(j_ninf)) <= hu and not (set(to_i(j_inf)) | set(to_i(j_nan))) & hu, u
    assert not np.any(h["seq_id"] == seq[2]), "the all-zero unit reports hits"
    # -inf everywhere: every evaluated bin above -inf is a hit, and the unit that is itself -inf still has none
    p, h = _check(n, x, np.full((1, n), -np.inf, np.float32), 0.0, want_spectrum=p_fixed)
    assert len(h) == 3 * ev_j.size and not np.any(h["seq_id"] == seq[2])
    # a threshold that sends baseline + threshold to +inf (3e38 + 3e38 overflows): only the -inf entries, which stay -inf, can hit
    baseline[:, j_nan] = np.float32(3e38)
    p, h = _check(n, x, baseline, 3e38, want_spectrum=p_fixed)
    assert len(h) == 3 * j_ninf.size and set(h["i"]) == set(to_i(j_ninf))


def _learn(n, flags, xs, x_tone, table_size, first):
    """set_baseline(rows, None), a submit, update(SET), two more with update(MAX), then every learnt input and the tone scene at
    threshold 0; returns what each step left"""
    units = xs[0].shape[0]
    got = dict(baselines=[], spectra=[], hits=[])
    with Plan(n, FS, 0.0, flags=flags, max_batch=units, detect=capi.DETECT_BASELINE, baseline=table_size) as plan:
        plan.set_table(100e6 + 6e6 * np.arange(table_size))
        assert np.all(np.isposinf(plan.baseline()))
        for k, x in enumerate(xs):
            _submit(plan, 0, x, first_index=first)
            p, h, t = plan.collect(0)
            if k == 0:
                assert len(h) == 0 and not t.any(), "an armed baseline of +inf lets a bin through"
            plan.update_baseline(0, capi.BASELINE_SET if k == 0 else capi.BASELINE_MAX)
            got["spectra"].append(p)
            got["baselines"].append(plan.baseline())
        assert plan.baseline(1, 2).tobytes() == got["baselines"][-1][1:3].tobytes()
        for x in list(xs) + [x_tone]:
            _submit(plan, 0, x, first_index=first)
            p, h, t = plan.collect(0)
            got["spectra"].append(p)
            got["hits"].append(h.copy())
        got["baselines"].append(plan.baseline())
    return got


@pytest.mark.parametrize("n", [64, 1001, 4096])
def test_learn_then_detect(built_lib, n):
    units, first = 5, 3
    rows = units + 2  # an indexed run that wraps: units 0 ... 4 read rows 3 4 5 6 0; rows 1 and 2 are never named
    xs = [_spectrum(n, units, seed=n + 50 + k)[0] for k in range(3)]
    j_tone = n // 8  # in band, away from the DC hole
    x_tone = np.array(xs[0])
    x_tone[1] += (0.5 * np.exp(2j * np.pi * j_tone * np.arange(n) / n)).astype(np.complex64)
    got = _learn(n, BOTH, xs, x_tone, rows, first)
    named = (first + np.arange(units)) % rows
    unnamed = np.setdiff1d(np.arange(rows), named)
    s = got["spectra"]
    b0 = got["baselines"][0]  # after SET: the first spectrum in the rows its units named, byte for byte; the others still +inf
    assert b0[named].tobytes() == s[0].tobytes() and np.all(np.isposinf(b0[unnamed]))
    want = baseline_ref.update(np.full((rows, n), np.inf, np.float32), s[0], first, capi.BASELINE_SET)
    assert baseline_ref.same_bits(b0, want)
    for k in (1, 2):  # max-hold, every bin, masked ones included
        want = baseline_ref.update(want, s[k], first, capi.BASELINE_MAX)
        assert baseline_ref.same_bits(got["baselines"][k], want), k
    assert not baseline_ref.same_bits(got["baselines"][2], got["baselines"][0])
    assert baseline_ref.same_bits(got["baselines"][3], want)  # detecting leaves the baseline as it is
    for k in range(3):  # every learnt input again: nothing exceeds its own maximum
        assert s[3 + k].tobytes() == s[k].tobytes() and len(got["hits"][k]) == 0, k
    table = 100e6 + 6e6 * np.arange(rows)
    want_h, _ = baseline_ref.detect(s[6], want, first, 0.0, table[named], None, FS)
    baseline_ref.assert_same_records(got["hits"][3], want_h, f"n {n}: the tone against the learnt baseline")
    h = got["hits"][3]
    assert len(h) > 0 and np.all(h["seq_id"] == 1)
    assert (j_tone + n - n // 2) % n in set(h["i"]), "the tone's peak bin is not among the hits"
    only = _learn(n, capi.OUT_HITS, xs, x_tone, rows, first)  # hits only: the detect kernel's own copy of the spectrum is what is learnt
    for k in range(4):
        assert only["baselines"][k].tobytes() == got["baselines"][k].tobytes(), k
    for k in range(4):
        assert only["hits"][k].tobytes() == got["hits"][k].tobytes(), k


def _status(call, *a, **kw):
    with pytest.raises(capi.ScannerError) as e:
        call(*a, **kw)
    return e.value.status


def test_refusals_leave_the_plan_working(built_lib):
    n, units = 1024, 4
    x, p_fixed = _spectrum(n, units, seed=61)
    _, baseline = _spectrum(n, units, seed=62)

    def still_works(plan):
        _submit(plan, 0, x)
        p, h, t = plan.collect(0)
        want_h, want_t = baseline_ref.detect(p, plan.baseline(), 0, 0.0, None, None, FS)
        baseline_ref.assert_same_records(h, want_h, "after a refusal")
        assert p.tobytes() == p_fixed.tobytes() and len(h) > 0

    with Plan(n, FS, 0.0, max_batch=units, detect=capi.DETECT_BASELINE) as plan:
        assert _status(_submit, plan, 0, x) == capi.E_STATE  # no baseline
        assert _status(plan.update_baseline, 0, capi.BASELINE_MAX) == capi.E_STATE
        assert _status(plan.collect_floor, 0) == capi.E_INVALID
        assert _status(plan.set_floor_window, 16, 2) == capi.E_INVALID
        plan._baseline_rows = 1
        assert _status(plan.baseline) == capi.E_INVALID  # nothing to read
        plan.set_baseline(baseline)
        assert _status(plan.update_baseline, 0, capi.BASELINE_MAX) == capi.E_STATE  # never submitted
        assert _status(plan.update_baseline, 1, capi.BASELINE_SET) == capi.E_STATE
        still_works(plan)
        _submit(plan, 1, x)  # a slot pending
        assert _status(plan.set_baseline, baseline) == capi.E_STATE
        assert _status(plan.set_baseline, 0) == capi.E_STATE
        assert _status(plan.update_baseline, 0, capi.BASELINE_MAX) == capi.E_STATE
        plan.collect(1)
        assert plan.baseline().tobytes() == baseline.tobytes()
        assert _status(plan.update_baseline, 0, 2) == capi.E_INVALID  # an unknown op
        assert _status(plan.baseline, units, 1) == capi.E_INVALID  # past the end
        assert _status(plan.baseline, 1, units) == capi.E_INVALID
        assert _status(plan.baseline, 0xFFFFFFFF, 2) == capi.E_INVALID
        assert plan.baseline(units, 0).shape == (0, n)
        still_works(plan)
        plan.set_baseline(baseline[:3])  # units > rows
        still_works(plan)
        assert _status(plan.update_baseline, 0, capi.BASELINE_MAX) == capi.E_INVALID
        assert plan.baseline().tobytes() == baseline[:3].tobytes()
        plan.set_table(100e6 + 6e6 * np.arange(5))  # an indexed submit: rows neither 1 nor the table's 5
        assert _status(_submit, plan, 0, x, first_index=1) == capi.E_STATE
        still_works(plan)
        plan.set_baseline(baseline[:1])
        _submit(plan, 0, x, first_index=1)  # one row serves every entry
        assert len(plan.collect(0)[1]) > 0
        assert _status(plan.collect_floor, 0) == capi.E_INVALID
        plan.set_baseline(0)  # dropped: as at first
        assert _status(_submit, plan, 0, x) == capi.E_STATE
        plan.set_baseline(baseline)
        still_works(plan)
    with Plan(n, FS, 0.0, max_batch=units) as plan:  # a fixed plan has no baseline
        assert _status(plan.set_baseline, baseline) == capi.E_INVALID
        assert _status(plan.update_baseline, 0, capi.BASELINE_SET) == capi.E_INVALID
        plan._baseline_rows = 1
        assert _status(plan.baseline) == capi.E_INVALID


def test_signals_and_collect_more(built_lib):
    n, units = 4096, 4
    x, _ = _spectrum(n, units, seed=71)
    _, baseline = _spectrum(n, units, seed=72)
    with Plan(n, FS, 2.0, max_batch=units, max_hits=256, detect=capi.DETECT_BASELINE, baseline=baseline) as plan:
        _submit(plan, 0, x)
        p, h, t = plan.collect(0)  # (more hits than max_hits: the rest comes through scn_collect_more)
        want_h, _ = baseline_ref.detect(p, baseline, 0, 2.0, None, None, FS)
        assert len(h) > 4 * 256
        baseline_ref.assert_same_records(h, want_h, "the whole list through collect_more")
        baseline_ref.assert_same_records(plan.collect_more(0, 100, 700), want_h[100:800], "a window of it")
        assert np.array_equal(plan.hits_view(0), h[:256])
        got = plan.collect_signals(0, max_gap=2)
    signals_ref.assert_same(got, capi.signals_from_hits(h, n, FS, 2), "GPU signals against scn_signals_from_hits")
    assert int(got["n_hits"].sum()) == len(h)


def test_two_slots_in_flight_read_different_rows(built_lib):
    """SCN_PLAN_OVERLAP_SLOTS: two indexed submits pending on streams of their own, each against its own run of the rows"""
    n, units = 4096, 3
    xs = [_spectrum(n, units, seed=81 + k)[0] for k in range(2)]
    rows = 2 * units
    baseline = np.repeat(np.linspace(-3.0, 3.0, rows).astype(np.float32)[:, None], n, axis=1)
    table = 100e6 + 6e6 * np.arange(rows)
    with Plan(n, FS, 0.0, max_batch=units, flags=BOTH | capi.PLAN_OVERLAP_SLOTS, detect=capi.DETECT_BASELINE, baseline=baseline) as plan:
        plan.set_table(table)
        for rep in range(2):  # the second round reuses both slots (the other generation of regions and counts)
            firsts = [(rep + units * k) % rows for k in range(2)]
            for k in range(2):
                _submit(plan, k, xs[k ^ rep], first_index=firsts[k])
            for k in range(2):
                p, h, t = plan.collect(k)
                fc = table[(firsts[k] + np.arange(units)) % rows]
                want_h, want_t = baseline_ref.detect(p, baseline, firsts[k], 0.0, fc, None, FS)
                baseline_ref.assert_same_records(h, want_h, f"round {rep} slot {k}")
                assert np.array_equal(t, want_t) and len(h) > 0
