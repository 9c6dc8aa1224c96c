"""The trace emitters on the GPU (scn_plan_trace_emitters, scn_plan_merge_trace; scn_emitters.hip).  Every expectation is an equality
of whole record arrays, byte for byte, with the host form (capi.trace_emitters), which is fed the plan's own trace() read-out of the
same window: the list is a pure function of the window (integers, compares and the spread's one subtraction), so there is no
tolerance and nothing exempt.  Where a case has an answer that can be said in a line -- a number of records, a peak cell -- it is
asserted beside the equality.

Cells are planted with merge_trace on a fresh set_trace: merged into an empty trace, a NaN-free window arrives bit for bit.  T is the
launcher's tile (tests/emitters_ref.py): a wave's cells, four tiles per workgroup; the kernels have no grid loop."""
import ctypes as C

import numpy as np
import pytest

from scanner_amd import Plan, capi, synth
from tests import emitters_ref as ref
from tests import trace_ref
from tests.test_floor_gpu import _noise, _straddling, _submit

pytestmark = pytest.mark.gpu

FS = 8000000
T = ref.TILE
F0, HZ = 433000000, 12500
MAX, MIN, SPREAD = capi.TRACE_LINE_MAX, capi.TRACE_LINE_MIN, capi.TRACE_LINE_SPREAD
INF = np.float32(np.inf)
QUIET = dict(threshold=1e9)


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.ScannerError as e:
        return e.status
    return capi.OK


def _plan(**kw):
    return Plan(16, FS, max_batch=1, **QUIET, **kw)


def _plant(plan, trace, f0=F0, hz=HZ):
    """a fresh trace of the window's size holding exactly `trace`"""
    plan.set_trace(f0, hz, trace[0].size)
    plan.merge_trace(*trace)
    assert trace_ref.same(plan.trace(), trace)


def _level(cells, on, hi=-20.0, lo=-90.0, count=3):
    """max = hi where `on` (indices or a mask), lo elsewhere; min 5 dB below; every cell counted"""
    mx = np.full(cells, lo, np.float32)
    mx[on] = hi
    return mx, (mx - np.float32(5)).astype(np.float32), np.full(cells, count, np.uint64)


def _check(plan, line, thr, gap=0, win=(0, None), f0=F0, hz=HZ, n=None, **answers):
    """the GPU list of the window win = (first cell, cells) against the host form on the plan's read-out of it; n: the number of
    records; answers: fields of record 0"""
    got = plan.trace_emitters(thr, line, gap, *win)
    readout = plan.trace(*win)
    want = capi.trace_emitters(readout, f0, hz, line, thr, gap, win[0]) if readout[0].size else np.zeros(0, capi.EMITTER_DTYPE)
    assert ref.same(got, want), (line, thr, gap, win, ref.describe(got, want))
    assert plan.last_n_emitters == want.size
    if n is not None:
        assert want.size == n, (want.size, n)
    for k, v in answers.items():
        assert want[0][k] == v, (k, want[0][k], v)
    return got


@pytest.mark.parametrize("cells", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_window_sizes(built_lib, cells):
    trace = ref.seeded_trace(cells, cells, p_empty=0.1)
    with _plan() as plan:
        _plant(plan, trace)
        for line, thr in ((MAX, -55.0), (MIN, -62.0), (SPREAD, 4.0)):
            for gap in (0, 1, 5):
                got = _check(plan, line, thr, gap)
                assert ref.same(got, ref.emitters(trace, F0, HZ, line, thr, gap))
        filled = int((trace[2] != 0).sum())
        got = _check(plan, MAX, -INF, cells, n=min(1, filled))  # every non-empty cell, as one emitter
        assert filled == 0 or got[0]["n_cells"] == filled
        _plant(plan, _level(cells, np.arange(cells)))
        _check(plan, MAX, -50.0, 0, n=1, first_cell=0, last_cell=cells - 1, n_cells=cells, stop_hz=F0 + cells * HZ)


def test_run_shapes(built_lib):
    cells = 2 * T + 3
    with _plan() as plan:
        _plant(plan, _level(cells, np.arange(cells)))
        _check(plan, MAX, -50.0, 0, n=1, first_cell=0, last_cell=cells - 1, n_cells=cells, count=3 * cells)  # all on (and the storage's first use)
        _check(plan, MAX, -10.0, 0, n=0)  # none on
        _plant(plan, _level(cells, np.arange(0, cells, 2)))
        got = _check(plan, MAX, -50.0, 0, n=(cells + 1) // 2)  # alternating: the record storage grows from 1 to cells / 2 + 1
        assert np.array_equal(got["first_cell"], np.arange(0, cells, 2)) and np.all(got["n_cells"] == 1)
        _check(plan, MAX, -50.0, 1, n=1, n_cells=(cells + 1) // 2, last_cell=cells - 1)
        _check(plan, MAX, -50.0, 0, n=(cells + 1) // 2)  # and back: every call recomputes


def test_tile_seams(built_lib):
    cells = 3 * T + 5
    with _plan() as plan:
        _plant(plan, _level(cells, np.arange(T // 2, 2 * T + T // 2)))
        _check(plan, MAX, -50.0, 0, n=1, first_cell=T // 2, last_cell=2 * T + T // 2 - 1, n_cells=2 * T)  # one run through three tiles
        for gap in (0, 1, 31, 32, 63, 64, T):
            for seam in (T, 2 * T):
                a = seam - 1 - gap // 2  # two on cells astride the seam ...
                _plant(plan, _level(cells, [a, a + gap + 1]))
                _check(plan, MAX, -50.0, gap, n=1, first_cell=a, last_cell=a + gap + 1, n_cells=2)  # ... at max_gap + 1: one emitter
                _plant(plan, _level(cells, [a, a + gap + 2]))
                _check(plan, MAX, -50.0, gap, n=2, first_cell=a, last_cell=a, n_cells=1)  # ... at max_gap + 2: two
        _plant(plan, _level(cells, [T - 1, 2 * T]))  # a wholly off tile between two on cells
        _check(plan, MAX, -50.0, T - 1, n=2)
        _check(plan, MAX, -50.0, T, n=1)
        for gap in (cells, 0xFFFFFFFF):
            _plant(plan, _level(cells, [0, cells - 1]))
            _check(plan, MAX, -50.0, gap, n=1, first_cell=0, last_cell=cells - 1, n_cells=2, count=6)
        _check(plan, MAX, -50.0, cells - 3, n=2)
        _check(plan, MAX, -50.0, cells - 2, n=1)


def test_peak(built_lib):
    cells = 3 * T
    with _plan() as plan:
        run = np.arange(10, 2 * T + 100)
        mx, mn, ct = _level(cells, run)
        mx[[T - 3, T + 70, 2 * T + 5]] = -7.0  # equal largest values in three tiles of one emitter: the lowest cell
        mn[T - 3] = -33.0
        _plant(plan, (mx, mn, ct))
        _check(plan, MAX, -50.0, 0, n=1, peak_cell=T - 3, peak_db=np.float32(-7.0), peak_other_db=np.float32(-33.0), peak_hz=F0 + (T - 3) * HZ)
        mx[2 * T + 99] = 1.0  # on the emitter's last cell
        _plant(plan, (mx, mn, ct))
        _check(plan, MAX, -50.0, 0, n=1, peak_cell=2 * T + 99)
        mx[10] = 1.0  # and, equal, on its first
        _plant(plan, (mx, mn, ct))
        _check(plan, MAX, -50.0, 0, n=1, peak_cell=10)
        mx[T + 1] = INF
        _plant(plan, (mx, mn, ct))
        _check(plan, MAX, -50.0, 0, n=1, peak_cell=T + 1, peak_db=INF)
        z = _level(cells, run, hi=-0.0, lo=-90.0)  # -0.0 everywhere, +0.0 late: +0.0 is the larger key
        z[0][2 * T + 7] = 0.0
        _plant(plan, z)
        got = _check(plan, MAX, -50.0, 0, n=1, peak_cell=2 * T + 7)
        assert got["peak_db"].view(np.uint32)[0] == 0
        z[0][2 * T + 7] = -0.0
        _plant(plan, z)
        got = _check(plan, MAX, -50.0, 0, n=1, peak_cell=10)
        assert got["peak_db"].view(np.uint32)[0] == 0x80000000
        got = _check(plan, MIN, -50.0, 0, n=1, peak_cell=10, peak_db=np.float32(-5.0))  # MIN: the other extreme is the cell's max
        assert got["peak_other_db"].view(np.uint32)[0] == 0x80000000


def test_values(built_lib):
    cells = T + 9
    tiny, tiny15 = np.uint32(0x00800000).view(np.float32), np.uint32(0x00C00000).view(np.float32)  # 2^-126, 1.5 * 2^-126
    mx, mn, ct = _level(cells, np.arange(0, cells, 3), hi=-20.0)
    mx[5:9], mn[5:9] = -INF, -INF            # -inf cells (|X| = 0 was folded): spread NaN
    mx[20], mn[20] = INF, INF                # inf - inf: NaN
    mx[21], mn[21] = INF, -INF               # spread +inf
    mx[30], mn[30], ct[30] = -1.5, -1.5, 1   # one value folded: spread 0.0, off at threshold 0
    mx[31], mn[31] = tiny15, tiny            # a denormal spread, 2^-127: on at threshold 0
    mx[40:50], mn[40:50], ct[40:50] = -INF, INF, 0  # empty cells amid on cells
    mx[50:60] = -20.0
    ct[60:70] = 1 << 40                      # counts beyond 32 bits, summed
    mx[60:70] = -20.0
    with _plan() as plan:
        _plant(plan, (mx, mn, ct))
        for line in (MAX, MIN, SPREAD):
            for thr in (-INF, INF, -20.0, np.nextafter(np.float32(-20.0), -INF), 0.0, -0.0, 5.0, np.nextafter(np.float32(5.0), -INF), -25.0):
                for gap in (0, 2, 10):
                    _check(plan, line, thr, gap)
        assert _check(plan, MAX, INF).size == 0 and _check(plan, SPREAD, INF).size == 0
        got = _check(plan, MAX, -20.0, 0)  # a value equal to the threshold is off: the +inf cells, -1.5 and 1.5 * 2^-126 remain
        assert got["first_cell"].tolist() == [20, 30] and got["last_cell"].tolist() == [21, 31]
        got = _check(plan, MAX, np.nextafter(np.float32(-20.0), -INF), 0)  # one ulp below: on
        assert got.size > 10 and 50 in got["first_cell"] and got[got["first_cell"] == 50][0]["count"] == 10 * 3 + 10 * (1 << 40)
        got = _check(plan, MAX, -INF, 0)  # every non-empty cell whose value is not -inf
        assert got["first_cell"].tolist() == [0, 9, 50] and got["last_cell"].tolist() == [4, 39, cells - 1]
        got = _check(plan, SPREAD, 0.0, 0)
        assert got["first_cell"].tolist()[:5] == [0, 9, 21, 31, 50] and got["last_cell"].tolist()[:4] == [4, 19, 29, 39]  # 30 (0.0) is off, 31 on
        got = _check(plan, SPREAD, 0.0, 0, win=(31, 1), n=1)
        assert got["peak_db"].view(np.uint32)[0] == 0x00400000 and got["peak_other_db"].view(np.uint32)[0] == 0x00C00000  # 2^-127, not flushed
        _check(plan, SPREAD, 0.0, 0, win=(30, 1), n=0)
        got = _check(plan, SPREAD, -INF, 0)  # -inf - -inf and inf - inf are NaN: off even here
        assert got["first_cell"].tolist()[:4] == [0, 9, 21, 50] and got["last_cell"].tolist()[:3] == [4, 19, 39]


def test_windows_and_pages(built_lib):
    cells = 2 * T + 300
    on = np.zeros(cells, bool)
    on[np.arange(0, cells, 7)] = True
    on[T - 40:T + 60] = True  # a run through the seam, which the windows below cut
    on[1500:1510] = True
    with _plan() as plan:
        _plant(plan, _level(cells, on))
        for first_cell, n in ((0, cells), (1, cells - 1), (37, T), (T - 10, 30), (T + 59, 2), (T + 60, 5), (cells - 1, 1), (999, T + 77), (T + 3, 0)):
            for gap in (0, 6, 7):
                _check(plan, MAX, -50.0, gap, win=(first_cell, n))
        got = _check(plan, MAX, -50.0, 0, win=(T - 10, 30), n=1, first_cell=T - 10, last_cell=T + 19)  # cut at both edges
        assert got[0]["start_hz"] == F0 + (T - 10) * HZ and got[0]["stop_hz"] == F0 + (T + 20) * HZ
        assert _check(plan, MAX, -50.0, 0, win=(T + 3, 0)).size == 0
        for bad in ((0, cells + 1), (cells, 1), (cells + 1, 0), (0xFFFFFFFF, 2)):
            assert _status(plan.trace_emitters, -50.0, MAX, 0, *bad) == capi.E_INVALID, bad
        # pages
        whole = _check(plan, MAX, -50.0, 0)
        total = whole.size
        assert total > 300
        for cap in (1, 7, total):
            pages = []
            for first in range(0, total, cap):
                out, n = np.zeros(cap, capi.EMITTER_DTYPE), C.c_uint32()
                st = plan._L.scn_plan_trace_emitters(plan.handle, 0, cells, MAX, -50.0, 0, first, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
                assert n.value == total and st == (capi.E_TRUNCATED if first + cap < total else capi.OK), (first, cap, st)
                pages.append(out[: min(cap, total - first)])  # (the records stored with SCN_E_TRUNCATED are valid)
            assert ref.same(np.concatenate(pages), whole), cap
        assert _status(plan.trace_emitters, -50.0, MAX, 0, first=3, cap=7) == capi.E_TRUNCATED and plan.last_n_emitters == total
        for first in (total, total + 1, 0xFFFFFFFF):
            assert plan.trace_emitters(-50.0, MAX, 0, first=first, cap=5).size == 0 and plan.last_n_emitters == total
        assert ref.same(plan.trace_emitters(-50.0, MAX, 0, first=total - 2, cap=1000), whole[total - 2:])


def test_the_largest_window(built_lib):
    cells = capi.TRACE_CELLS_MAX
    trace = ref.seeded_trace(cells, 7)
    with _plan() as plan:
        plan.set_trace(0, 0xFFFFFFFF, cells)
        plan.merge_trace(*trace)
        for line, thr, gap in ((MAX, -55.0, 0), (MIN, -66.0, 1), (SPREAD, 6.0, 3)):
            got = plan.trace_emitters(thr, line, gap)
            want = ref.emitters(trace, 0, 0xFFFFFFFF, line, thr, gap)
            assert want.size > cells // 32 and ref.same(got, want), (line, ref.describe(got, want))
        got = plan.trace_emitters(-INF, MAX, cells)  # and as one emitter
        assert ref.same(got, ref.emitters(trace, 0, 0xFFFFFFFF, MAX, -INF, cells)) and got.size == 1


def test_merge_trace(built_lib):
    n, units, cells = 1024, 4, 600
    centres = 100e6 + 6e6 * np.arange(units)
    f0, hz = 97000000, 30000
    rng = np.random.default_rng(3)
    src = list(ref.seeded_trace(cells, 11, p_empty=0.3))
    src[0][:8] = [INF, -INF, 0.0, -0.0, INF, -0.0, 0.0, 5.0]
    src[1][:8] = [INF, -INF, -0.0, -0.0, -INF, 0.0, 0.0, 5.0]
    src[2][:8] = [1, 1, 2, 1, 2, 2, 1, 0]
    src[2][8:200] = (np.uint64(1) << np.uint64(32)) - rng.integers(0, 3, 192).astype(np.uint64)  # carries past 2^32 when merged twice
    src = tuple(src)
    with Plan(n, FS, max_batch=units, **QUIET) as plan:
        plan.set_trace(f0, hz, cells)
        plan.merge_trace(*src)  # into an empty trace: the window itself
        assert trace_ref.same(plan.trace(), src)
        plan.merge_trace(*src)
        want = tuple(a.copy() for a in src)
        capi.trace_merge(want, src)
        assert trace_ref.same(plan.trace(), want) and int(want[2][8:200].min()) > 1 << 32
        plan.set_trace(f0, hz, cells)  # into a folded one
        _submit(plan, 0, _noise(n, units, seed=2), center_freqs=centres)
        plan.collect(0)
        plan.update_trace(0)
        folded = plan.trace()
        assert folded[2].sum() > 0
        plan.merge_trace(*src)
        want = tuple(a.copy() for a in folded)
        capi.trace_merge(want, src)
        assert trace_ref.same(plan.trace(), want)
        mid = tuple(a[100:177] for a in src)  # a window in the middle
        plan.merge_trace(*mid, first=301)
        capi.trace_merge(tuple(a[301:378] for a in want), mid)
        assert trace_ref.same(plan.trace(), want)
        plan.merge_trace(*(a[:0] for a in src), first=cells)  # no cell: SCN_OK
        # a NaN in either source array: refused, nothing changed
        for which in (0, 1):
            for nan in (np.float32(np.nan), np.uint32(0xFFC00001).view(np.float32)):
                bad = [a.copy() for a in mid]
                bad[which][76] = nan
                assert _status(plan.merge_trace, *bad, first=5) == capi.E_INVALID and b"NaN" in plan._L.scn_last_error()
        assert trace_ref.same(plan.trace(), want)
        for first, k in ((cells, 1), (cells - 76, 77), (0xFFFFFFFF, 2)):
            assert _status(plan.merge_trace, *(a[:k] for a in mid), first=first) == capi.E_INVALID, (first, k)
        assert plan._L.scn_plan_merge_trace(plan.handle, 0, 4, None, mid[1].ctypes.data_as(C.c_void_p), mid[2].ctypes.data_as(C.c_void_p)) == capi.E_INVALID
        assert trace_ref.same(plan.trace(), want)
        plan.set_trace(0, 0, 0)
        assert _status(plan.merge_trace, *mid) == capi.E_STATE


def test_state(built_lib):
    n, units = 1024, 4
    centres = 100e6 + 6e6 * np.arange(units)
    trace = _level(500, np.arange(100, 140))
    with _plan() as plan:
        assert _status(plan.trace_emitters, -50.0) == capi.E_STATE and _status(plan.trace_emitters, -50.0, MAX, 0, 0, 0) == capi.E_STATE  # no trace
        assert _status(plan.merge_trace, *trace) == capi.E_STATE
        assert _status(plan.trace_emitters, -50.0, 3) == capi.E_INVALID and _status(plan.trace_emitters, float("nan")) == capi.E_INVALID
        _plant(plan, trace)
        assert _status(plan.trace_emitters, -50.0, 3) == capi.E_INVALID and _status(plan.trace_emitters, float("nan")) == capi.E_INVALID
        assert _status(plan.trace_emitters, -50.0, 0xFFFFFFFF) == capi.E_INVALID
        n_out = C.c_uint32()
        assert plan._L.scn_plan_trace_emitters(plan.handle, 0, 500, MAX, -50.0, 0, 0, None, 1, C.byref(n_out)) == capi.E_INVALID
        assert plan._L.scn_plan_trace_emitters(plan.handle, 0, 500, MAX, -50.0, 0, 0, None, 0, None) == capi.E_INVALID
        assert plan.trace_emitters(-50.0, cells=0).size == 0 and plan.last_n_emitters == 0  # cells == 0: SCN_OK, no emitter
        _check(plan, MAX, -50.0, n=1)
        plan.set_trace(0, 0, 0)
        assert _status(plan.trace_emitters, -50.0) == capi.E_STATE
    for kw in (dict(mode=capi.MODE_TIME_DOMAIN), dict(flags=capi.OUT_SPECTRUM), dict(flags=capi.OUT_HITS)):  # plans that cannot have a trace
        with _plan(**kw) as plan:
            assert _status(plan.trace_emitters, -50.0) == capi.E_INVALID and _status(plan.merge_trace, *trace) == capi.E_INVALID, kw
    # beside a pending slot: both calls succeed, and the slot's later collect is what a twin plan's is
    xa, xb = synth.cfloat_batch(n, units, seed=31), synth.cfloat_batch(n, units, seed=32)
    kw = dict(threshold=2.0, max_batch=units)
    with Plan(n, FS, **kw) as solo:
        _submit(solo, 0, xb, center_freqs=centres)
        p_solo, h_solo, t_solo = solo.collect(0)
        assert len(h_solo) > 0
    with Plan(n, FS, **kw) as plan:
        plan.set_trace(97000000, 64 * (FS // n) + 7, 40)
        _submit(plan, 0, xa, center_freqs=centres)
        plan.collect(0)
        plan.update_trace(0)
        _submit(plan, 1, xb, center_freqs=centres)  # slot 1 stays pending
        before = plan.trace()
        src = _level(40, np.arange(3, 9), hi=90.0)
        plan.merge_trace(*src)
        want = tuple(a.copy() for a in before)
        capi.trace_merge(want, src)
        assert trace_ref.same(plan.trace(), want)
        _check(plan, MAX, 50.0, 0, f0=97000000, hz=64 * (FS // n) + 7, n=1, first_cell=3, last_cell=8)
        pb, hb, tb = plan.collect(1)
        assert pb.tobytes() == p_solo.tobytes() and hb.tobytes() == h_solo.tobytes() and np.array_equal(tb, t_solo)


def test_end_to_end_one_emitter_across_a_table_seam(built_lib):
    """the point of the feature: a block of tones that straddles the seam between two table entries is two signals -- one per unit --
    and ONE emitter of the trace, however often it is folded"""
    n, units = 1024, 3
    bin_step = FS // n
    ev = np.flatnonzero(trace_ref.evaluated(n))
    i_lo, i_hi = int(ev[0]), int(ev[-1])
    span = i_hi - i_lo + 1
    table = 100e6 + float(span * bin_step) * np.arange(units)  # the evaluated bands abut: unit u + 1's first bin follows unit u's last
    f0 = int(trace_ref.bin_freqs(n, FS, table[0])[i_lo])
    assert int(trace_ref.bin_freqs(n, FS, table[1])[i_lo]) == int(trace_ref.bin_freqs(n, FS, table[0])[i_hi]) + bin_step
    # noise whose dB values (10 log10 |X|) lie around 0, and tones of |X| = 10^4, 40 dB above: a tone on bin i of amplitude A with
    # alternating signs from bin to bin gives |X| = A n under the Blackman-Harris window (its four coefficients add up to 1)
    x = _straddling(n, units, seed=77)
    t = np.arange(n)
    for u, bins in ((0, np.arange(i_hi - 19, i_hi + 1)), (1, np.arange(i_lo, i_lo + 20))):
        for i in bins:
            j = (i + n // 2) % n
            x[u] += np.complex64((-1.0) ** int(i) * 1e4 / n) * np.exp(2j * np.pi * j * t / n).astype(np.complex64)
    threshold = 20.0  # halfway
    with Plan(n, FS, threshold=threshold, max_batch=units) as plan:
        plan.set_table(table)
        plan.set_trace(f0, bin_step, units * span)
        _submit(plan, 0, x, first_index=0)
        p, hits, _ = plan.collect(0)
        signals = plan.collect_signals(0, max_gap=8)
        assert signals.size == 2 and signals["seq_id"].tolist() == [0, 1], signals  # one per unit: a signal never spans two units
        assert signals[0]["last_i"] == i_hi and signals[1]["first_i"] == i_lo and min(signals["n_hits"]) >= 20
        assert set(hits["seq_id"].tolist()) == {0, 1}
        plan.update_trace(0)
        got = _check(plan, MAX, threshold, 8, f0=f0, hz=bin_step, n=1)
        e = got[0]
        assert e["start_hz"] <= hits["freq_hz"].min() and hits["freq_hz"].max() < e["stop_hz"]
        assert e["first_cell"] <= span - 20 and e["last_cell"] >= span + 19 and e["n_cells"] == len(hits) and e["count"] == e["n_cells"]
        assert e["start_hz"] == f0 + int(e["first_cell"]) * bin_step and e["stop_hz"] == f0 + (int(e["last_cell"]) + 1) * bin_step
        plan.update_trace(0)  # the same submit folded again: the same emitter, counted twice
        again = _check(plan, MAX, threshold, 8, f0=f0, hz=bin_step, n=1)
        want = got.copy()
        want["count"] *= 2
        assert ref.same(again, want)
