"""The hit history on the GPU (scn_plan_set_history, scn_plan_update_history, scn_plan_get_history, scn_collect_confirmed;
scn_history.hip).  Every assertion is an equality.  tests/history_ref.py, the numpy model written from the definition, is fed the
PLAN'S OWN collected hit list of each submit: the fold is a pure function of that list -- which the other suites hold -- so there
is no tolerance and no guard band.  A scene is a sequence of sweeps of fresh seeded noise on one plan; after each sweep: collect,
update_history, then
  1. plan.history() equals the model, for all rows, including the rows no unit touched;
  2. collect_confirmed equals the model's subsequence for several (m, window);
  3. at (1, 1) it equals the collected list byte for byte;
  4. paging with a cap smaller than the total returns the same list (`first`, SCN_E_TRUNCATED).
In the floor-plan scenes of n >= 128 the model's (2, 2) list must hold between 10 % and 90 % of the collected list in every sweep
after the second -- independent half-density sweeps give about half (tests/test_history_cpu.py holds that on synthetic lists) --,
asserted on the model's output before the device is looked at: the comparison cannot pass on empty or full lists alone."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (the plans' device memory)

from scanner_amd import Plan, capi
from tests import history_ref
from tests import tolerances as tol
from tests.test_floor_gpu import _straddling, _submit

pytestmark = pytest.mark.gpu

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS
MW = [(1, 1), (2, 2), (2, 3), (3, 5), (32, 32), (1, 32)]
FLOOR = dict(threshold=0.0, detect=capi.DETECT_FLOOR)  # hits: the evaluated bins strictly above the unit's median -- about half


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.ScannerError as e:
        return e.status
    return capi.OK


def _paged(plan, slot, m, window, cap):
    """the confirmed list read `cap` records at a time through the C-ABI itself: every page but the last is SCN_E_TRUNCATED"""
    pages, first, total = [], 0, C.c_uint32()
    while True:
        out = np.zeros(cap, capi.HIT_DTYPE)
        st = plan._L.scn_collect_confirmed(plan.handle, slot, m, window, first, out.ctypes.data_as(C.c_void_p), cap, C.byref(total))
        assert st == (capi.E_TRUNCATED if first + cap < total.value else capi.OK), (st, first, cap, total.value)
        pages.append(out[: max(0, min(cap, total.value - first))])
        first += cap
        if first >= total.value:
            return np.concatenate(pages)


class Scene:
    """one plan with a history and the model beside it"""

    def __init__(self, plan, rows):
        self.plan, self.rows = plan, rows
        plan.set_history(rows)
        self.hist, self.visits = history_ref.new(rows, plan.n)
        self.fractions = []  # the model's (2, 2) list over the collected list, per sweep

    def check_history(self):
        got_h, got_v = self.plan.history()
        assert np.array_equal(got_h, self.hist) and np.array_equal(got_v, self.visits)

    def folded(self, slot, hits, ids, first=0, mw=MW):
        """the slot was collected (`hits`, its units' ids `ids`) and folded: the model follows, then assertions 1 to 4"""
        plan, units = self.plan, len(ids)
        self.hist, self.visits = history_ref.fold(self.hist, self.visits, hits, units, first=first, seq_ids=ids)
        want = {k: history_ref.confirm(self.hist, hits, units, *k, first=first, seq_ids=ids) for k in mw}
        if (2, 2) in want and len(hits):
            self.fractions.append(len(want[(2, 2)]) / len(hits))
        self.check_history()                                                                   # 1
        for (m, window), w in want.items():
            got = plan.collect_confirmed(slot, m, window)
            assert plan.last_n_confirmed == len(w) and got.tobytes() == w.tobytes(), (m, window, len(got), len(w))  # 2
        assert plan.collect_confirmed(slot, 1, 1).tobytes() == hits.tobytes()                  # 3
        for (m, window), w in want.items():
            if (m, window) in ((1, 1), (2, 2)) and len(w) > 1:
                assert _paged(plan, slot, m, window, max(1, len(w) // 3)).tobytes() == w.tobytes()  # 4
                assert plan.collect_confirmed(slot, m, window, first=len(w) - 1).tobytes() == w[-1:].tobytes()
        return want

    def sweep(self, x, ids, slot=0, first=0, mw=MW, **submit_kw):
        _submit(self.plan, slot, x, **submit_kw)
        hits = self.plan.collect(slot)[1].copy()
        self.plan.update_history(slot)
        return hits, self.folded(slot, hits, ids, first=first, mw=mw)


def _seqs(nb, sweep):
    return 1000 + 3 * np.arange(nb, dtype=np.uint64) + np.uint64(100000 * sweep)


def _floor_scene(n, units, rows, sweeps, seed, dense_enough, **plan_kw):
    with Plan(n, FS, max_batch=units, **FLOOR, **plan_kw) as plan:
        scene = Scene(plan, rows)
        for sweep in range(sweeps):
            seq = _seqs(units, sweep)
            scene.sweep(_straddling(n, units, seed + sweep), seq, seq_ids=seq)
        if dense_enough:
            assert len(scene.fractions) == sweeps and all(0.1 <= f <= 0.9 for f in scene.fractions[2:]), scene.fractions
        assert scene.visits.tolist() == [sweeps] * units + [0] * (rows - units)
    return scene


# 16: a handful of evaluated bins, a bitmap of one word; 128: four bitmap words, a wave per unit, one 16-byte access per lane;
# 512: the largest wave-per-unit size, two accesses in flight; 1024: a workgroup of 256 per unit, one access; 4096: four in flight
@pytest.mark.parametrize("n", [16, 128, 512, 1024, 4096])
def test_sizes_and_teams(built_lib, n):
    _floor_scene(n, units=3, rows=5, sweeps=4, seed=10 * n, dense_enough=n >= 128)


# 1000: mixed radix, n % 4 == 0 but a last bitmap word of 8 bins; 1001: Bluestein, the 4-byte accesses, rows 4-byte aligned only;
# 8192: a workgroup of 1024 per unit
@pytest.mark.parametrize("n", [1000, 1001, 8192])
def test_other_sizes(built_lib, n):
    _floor_scene(n, units=3, rows=5, sweeps=3, seed=7 * n, dense_enough=True)


def test_65536(built_lib):
    """the four-step pair, a bitmap of 8 KiB, sixteen trips of the 1024-thread team"""
    _floor_scene(65536, units=1, rows=2, sweeps=1, seed=65536, dense_enough=False)


def test_many_units(built_lib):
    """more units than a launch has teams, so that the teams walk on with the grid's stride: the fold's grid is capped at what is
    resident (at most 8 workgroups of four waves on each of 256 CUs: 8192 units), the confirm kernels' at 8192 workgroups of four
    waves (32768 units).  Every unit has a row of its own; the last row is never visited."""
    _floor_scene(16, units=33000, rows=33001, sweeps=3, seed=33, dense_enough=True)


@pytest.mark.parametrize("extra", [dict(max_hits=64), dict(flags=BOTH | capi.PLAN_OVERLAP_SLOTS)])
def test_plan_options(built_lib, extra):
    """a plan that keeps only 64 records of its list -- the history and the confirmed list are made from ALL of the submit's hits --
    and one whose slots have streams of their own, where the side stream is the slot's"""
    _floor_scene(2048, units=3, rows=5, sweeps=3, seed=2048, dense_enough=True, **extra)


@pytest.mark.parametrize("threshold,full", [(-1e30, True), (1e30, False)])
def test_full_and_empty(built_lib, threshold, full):
    """every evaluated bin a hit -- the regions are full, stored == hit_region -- and none at all: zeros shift in, visits still grow"""
    n, units, rows, sweeps = 1024, 3, 5, 3
    evaluated = int(tol.evaluated_mask(n).sum())
    i_ev = np.flatnonzero(tol.evaluated_mask(n)[(np.arange(n) + n // 2) % n])
    with Plan(n, FS, threshold, max_batch=units) as plan:
        scene = Scene(plan, rows)
        for sweep in range(sweeps):
            seq = _seqs(units, sweep)
            hits, want = scene.sweep(_straddling(n, units, 500 + sweep), seq, seq_ids=seq)
            assert len(hits) == (units * evaluated if full else 0)
            assert len(want[(2, 2)]) == (len(hits) if sweep >= 1 else 0)
        word = (1 << sweeps) - 1 if full else 0
        expect = np.zeros((rows, n), np.uint32)
        expect[:units, i_ev] = word
        assert np.array_equal(scene.hist, expect) and scene.visits.tolist() == [sweeps] * units + [0] * (rows - units)


def test_rows_follow_the_table_and_wrap(built_lib):
    """an indexed submit from entry 3 of a table of 5: its units visit rows 3, 4, 0; rows 1 and 2 stay as they were"""
    n, units, rows = 256, 3, 5
    with Plan(n, FS, max_batch=units, **FLOOR) as plan:
        plan.set_table(100e6 + 6e6 * np.arange(rows))
        scene = Scene(plan, rows)
        for sweep in range(4):
            first = 3 if sweep != 2 else 1  # (the third sweep visits rows 1, 2, 3)
            seq = _seqs(units, sweep) if sweep % 2 else None  # (without ids a unit's id is its index)
            scene.sweep(_straddling(n, units, 900 + sweep), history_ref.unit_ids(units, seq), first=first, first_index=first, seq_ids=seq)
        assert scene.visits.tolist() == [3, 1, 1, 4, 3]
        assert all(0.1 <= f <= 0.9 for f in scene.fractions[3:]), scene.fractions  # (the fourth sweep: rows visited twice before)


@pytest.mark.parametrize("units,rows", [(1, 1), (5, 5)])
def test_one_row_and_units_equal_to_rows(built_lib, units, rows):
    n = 128
    with Plan(n, FS, max_batch=units, **FLOOR) as plan:
        plan.set_table(100e6 + 6e6 * np.arange(7))
        scene = Scene(plan, rows)
        for sweep in range(3):
            seq = _seqs(units, sweep)
            # rows == 1 takes an indexed submit from anywhere in the table; units == rows a plain one
            kw = dict(first=4, first_index=4) if rows == 1 else {}
            scene.sweep(_straddling(n, units, 40 * rows + sweep), seq, seq_ids=seq, **kw)
        assert scene.visits.tolist() == [3] * rows and all(0.1 <= f <= 0.9 for f in scene.fractions[2:])


def test_depth_floor_plan(built_lib):
    """35 sweeps at n = 16: bit 31 is reached and falls off, with patterns that change from sweep to sweep"""
    n, units, rows = 16, 3, 5
    with Plan(n, FS, max_batch=units, **FLOOR) as plan:
        scene = Scene(plan, rows)
        top = False
        for sweep in range(35):
            seq = _seqs(units, sweep)
            _, want = scene.sweep(_straddling(n, units, 3000 + sweep), seq, seq_ids=seq)
            top = top or bool((scene.hist >> 31).any())
            assert sweep >= 31 or len(want[(32, 32)]) == 0
        assert top and scene.visits.tolist() == [35] * units + [0] * (rows - units)


def test_depth_32_of_32(built_lib):
    """every evaluated bin a hit in every sweep: (32, 32) confirms nothing before the 32nd visit and everything from it on"""
    n, units, rows = 16, 3, 3
    with Plan(n, FS, -1e30, max_batch=units, flags=capi.OUT_HITS) as plan:
        scene = Scene(plan, rows)
        for sweep in range(35):
            hits, want = scene.sweep(_straddling(n, units, 4000 + sweep), history_ref.unit_ids(units), mw=[(32, 32), (31, 32), (1, 1)])
            assert len(hits) == units * int(tol.evaluated_mask(n).sum())
            assert len(want[(32, 32)]) == (len(hits) if sweep >= 31 else 0) and len(want[(31, 32)]) == (len(hits) if sweep >= 30 else 0)
        assert int(scene.hist.max()) == 0xFFFFFFFF


def test_fixed_plan_with_and_without_spectrum(built_lib):
    """the fixed detector, spectrum + hits and hits only: the same lists, the same history"""
    n, units, rows, sweeps = 2048, 3, 4, 3
    hists = {}
    for flags in (BOTH, capi.OUT_HITS):
        with Plan(n, FS, 0.0, max_batch=units, flags=flags) as plan:  # (the noise straddles 0 dB: about half the bins are hits)
            scene = Scene(plan, rows)
            for sweep in range(sweeps):
                seq = _seqs(units, sweep)
                scene.sweep(_straddling(n, units, 7000 + sweep), seq, seq_ids=seq)
            assert all(0.1 <= f <= 0.9 for f in scene.fractions[2:]), scene.fractions
            hists[flags] = (scene.hist, scene.visits)
    assert np.array_equal(hists[BOTH][0], hists[capi.OUT_HITS][0]) and np.array_equal(hists[BOTH][1], hists[capi.OUT_HITS][1])


def test_baseline_plan(built_lib):
    n, units, rows = 512, 3, 5
    with Plan(n, FS, 0.0, max_batch=units, detect=capi.DETECT_BASELINE, baseline=np.zeros((rows, n), np.float32)) as plan:
        scene = Scene(plan, rows)
        for sweep in range(3):
            seq = _seqs(units, sweep)
            scene.sweep(_straddling(n, units, 8000 + sweep), seq, seq_ids=seq)
        assert all(0.1 <= f <= 0.9 for f in scene.fractions[2:]), scene.fractions


@pytest.mark.parametrize("given_ids", [True, False])
def test_averaged_plan(built_lib, given_ids):
    """average = 2: the units are the groups, a unit's id is that of its group's first buffer"""
    n, k, units, rows = 1024, 2, 3, 5
    nb = k * units
    with Plan(n, FS, max_batch=nb, average=k, **FLOOR) as plan:
        scene = Scene(plan, rows)
        for sweep in range(3):
            seq = _seqs(nb, sweep) if given_ids else None
            ids = seq[::k] if given_ids else np.arange(0, nb, k, dtype=np.uint64)  # (SCN_AVG_DWELL: group g = buffers g k ...)
            scene.sweep(_straddling(n, nb, 9000 + sweep), ids, seq_ids=seq)
        assert scene.visits.tolist() == [3] * units + [0] * (rows - units)
        assert all(0.1 <= f <= 0.9 for f in scene.fractions[2:]), scene.fractions


def test_fold_beside_a_pending_slot(built_lib):
    """slot 0 is collected and folded while slot 1 is pending: slot 1's spectrum and hits are those of a run in which nothing was
    ever folded; then slot 1's fold makes slot 0's no longer the latest"""
    n, units, rows = 4096, 3, 5
    x0, x1 = _straddling(n, units, 11), _straddling(n, units, 12)
    seq0, seq1 = _seqs(units, 0), _seqs(units, 1)
    with Plan(n, FS, max_batch=units, **FLOOR) as plain:  # no history, no fold
        _submit(plain, 0, x0, seq_ids=seq0)
        _submit(plain, 1, x1, seq_ids=seq1)
        plain.collect(0)
        p1_want, h1_want, t1_want = plain.collect(1)
    with Plan(n, FS, max_batch=units, **FLOOR) as plan:
        scene = Scene(plan, rows)
        _submit(plan, 0, x0, seq_ids=seq0)
        _submit(plan, 1, x1, seq_ids=seq1)
        h0 = plan.collect(0)[1].copy()
        plan.update_history(0)  # slot 1 is pending
        scene.folded(0, h0, seq0)
        p1, h1, t1 = plan.collect(1)
        assert p1.tobytes() == p1_want.tobytes() and h1.tobytes() == h1_want.tobytes() and np.array_equal(t1, t1_want)
        h1 = h1.copy()
        assert _status(plan.collect_confirmed, 1, 1, 1) == capi.E_STATE  # collected, not folded
        assert plan.collect_confirmed(0, 1, 1).tobytes() == h0.tobytes()  # slot 0's fold is still the latest
        plan.update_history(1)
        assert _status(plan.collect_confirmed, 0, 1, 1) == capi.E_STATE  # no longer
        scene.folded(1, h1, seq1)
        assert scene.visits.tolist() == [2] * units + [0] * (rows - units)
        plan.set_history(rows)  # a new history, a new epoch: slot 1's fold went into the old one
        assert _status(plan.collect_confirmed, 1, 1, 1) == capi.E_STATE and _status(plan.update_history, 1) == capi.E_STATE
        assert not plan.history()[0].any() and not plan.history()[1].any()


def test_refusals(built_lib):
    n, units, rows = 64, 3, 3
    x = _straddling(n, units + 1, 21)
    with Plan(n, FS, max_batch=units + 1, **FLOOR) as plan:
        _submit(plan, 0, x, units)
        plan.collect(0)
        assert _status(plan.update_history, 0) == capi.E_STATE                  # no history
        assert _status(plan.history, 0, 1) == capi.E_INVALID
        scene = Scene(plan, rows)
        assert _status(plan.update_history, 1) == capi.E_STATE                  # a slot never submitted
        assert _status(plan.collect_confirmed, 0, 1, 1) == capi.E_STATE         # confirm before fold
        for m, window in ((0, 1), (0, 0), (3, 2), (1, 33), (33, 33)):
            assert _status(plan.collect_confirmed, 0, m, window) == capi.E_INVALID, (m, window)
        _submit(plan, 1, x, units)
        assert _status(plan.update_history, 1) == capi.E_STATE                  # a pending slot
        assert _status(plan.collect_confirmed, 1, 1, 1) == capi.E_STATE
        h1 = plan.collect(1)[1].copy()
        _submit(plan, 2, x, units + 1)
        plan.collect(2)
        assert _status(plan.update_history, 2) == capi.E_INVALID                # units > rows
        assert _status(plan.history, 1, rows) == capi.E_INVALID                 # rows [1, 1 + 3) of 3
        scene.check_history()                                                   # nothing has changed: all zero, no visit
        plan.update_history(1)
        scene.folded(1, h1, history_ref.unit_ids(units))
        assert _status(plan.update_history, 1) == capi.E_STATE                  # fold twice
        plan.set_table(100e6 + 6e6 * np.arange(5))                              # (forgets the collected lists)
        assert _status(plan.update_history, 0) == capi.E_STATE
        _submit(plan, 0, x, 2, first_index=1)
        plan.collect(0)
        assert _status(plan.update_history, 0) == capi.E_STATE                  # indexed: 3 rows, a table of 5
        _submit(plan, 3, x, 0)
        plan.collect(3)
        plan.update_history(3)                                                  # zero units: SCN_OK and no visit
        assert _status(plan.update_history, 3) == capi.E_STATE
        scene.check_history()
        got_h, got_v = plan.history(1, 2)
        assert np.array_equal(got_h, scene.hist[1:]) and np.array_equal(got_v, scene.visits[1:])
    with Plan(n, FS, max_batch=units, mode=capi.MODE_TIME_DOMAIN) as plan:
        assert _status(plan.set_history, rows) == capi.E_INVALID and _status(plan.update_history, 0) == capi.E_INVALID
        assert _status(plan.collect_confirmed, 0, 1, 1) == capi.E_INVALID and _status(plan.history, 0, 0) == capi.E_INVALID
    with Plan(n, FS, max_batch=units, flags=capi.OUT_SPECTRUM) as plan:
        assert _status(plan.set_history, rows) == capi.E_INVALID and _status(plan.update_history, 0) == capi.E_INVALID
        assert _status(plan.collect_confirmed, 0, 1, 1) == capi.E_INVALID and _status(plan.history, 0, 0) == capi.E_INVALID
