"""tests/sequence_cases.py's committed seed list on the CPU: it covers what it is there for, the runner (tests/sequence_run.py) passes
against the model (tests/sequence_model.py) for every committed script -- so the scripts are legal under the header's rules and the
checker agrees with itself --, and the runner FAILS against eight deliberately broken models, each at the kind of step its fault must
show at: the CPU-side proof that tests/test_plan_sequences_gpu.py would fail on the state faults it is there for."""
import functools
import time

import numpy as np
import pytest

from scanner_amd import capi
from tests import sequence_cases as cases
from tests import sequence_run
from tests.sequence_model import ModelPlan, numpy_source


@functools.lru_cache(maxsize=None)
def _scripts():
    return [(seed, index, sc) for seed in cases.SEEDS for index, sc in enumerate(cases.draw(seed))]


def test_draw_is_deterministic_and_made_of_literals():
    seed = cases.SEEDS[0]
    a, b = cases.draw(seed), cases.draw(seed)
    assert repr(a) == repr(b) and len(a) == cases.SCRIPTS_PER_SEED
    assert eval(repr(a), {}) == a, "a script must survive repr(): that is how a failure is pasted into a regression test"


def test_the_committed_seeds_cover_what_they_are_there_for():
    got = cases.coverage([sc for _, _, sc in _scripts()])
    missing = cases.required() - got
    assert not missing, sorted(missing, key=str)
    # stated once more, without the helper: every (detector, size family) pair the header allows, each with its own plan
    pairs = {(sc["plan"]["detect"], cases.FAMILY_OF[sc["plan"]["n"]]) for _, _, sc in _scripts()}
    assert pairs == {(d, f) for d in cases.DETECTORS for f in cases.FAMILIES}
    refusals = sum(st["expect"] != capi.OK for _, _, sc in _scripts() for st in sc["steps"])
    assert len(_scripts()) / 6 <= refusals <= len(_scripts()), (refusals, len(_scripts()))  # about one per three scripts


def test_the_limits_of_a_script():
    for seed, index, sc in _scripts():
        p = sc["plan"]
        assert p["max_batch"] // p["average"] <= cases.max_units(p["n"]) and p["max_batch"] % p["average"] == 0, (seed, index)
        assert p["average"] == 1 or p["n"] in cases.FAMILIES["averaged"], (seed, index)
        assert len(sc["steps"]) <= 60, (seed, index)


@pytest.fixture(scope="module")
def source(built_lib, oracle_mod):
    return numpy_source(oracle_mod)


def test_the_runner_passes_against_the_model(source):
    """every committed script, the runner against ModelPlan itself; prints the references' CPU time per seed"""
    stats = sequence_run.new_stats()
    for seed in cases.SEEDS:
        t0 = time.perf_counter()
        for s, index, sc in _scripts():
            if s == seed:
                sequence_run.run(sc, lambda d: ModelPlan(d, source(d)), source, seed, index, stats)
        print(f"seed {seed}: {time.perf_counter() - t0:.2f} s of references on the CPU")
    print(stats)
    assert stats["scripts"] == len(_scripts()) and stats["exempt_records"] == 0 and stats["tolerances"] == 0
    assert stats["records"] > 0 and stats["signals"] > 0 and stats["floors"] > 0 and stats["baseline_floats"] > 0 and stats["special_units"] > 0


# ---- the checker sees state faults: one broken rule each ------------------------------------------------------------------------------
class KeepsTheOldWindow(ModelPlan):  # 1: a re-set window leaves the previous one's `need` in place
    def _new_window(self, train, guard):
        return self.window if self.window != (0, 0) and (train, guard) != (0, 0) else (train, guard)


class NoneIsTheLastWindow(ModelPlan):  # 2: (0, 0) does not return to the unit-wide floor
    def _new_window(self, train, guard):
        return self.window if (train, guard) == (0, 0) else (train, guard)


class RowIgnoresFirst(ModelPlan):  # 3: row u % rows
    def _rows_of(self, first, units, rows):
        return np.arange(units) % rows


class FoldsAnotherSlot(ModelPlan):  # 4: update_baseline takes the lowest slot that has something to fold
    def _fold_slot(self, slot):
        return next(s for s in range(capi.NUM_SLOTS) if self.slot[s].base is not None)


class MaxByFloatCompare(ModelPlan):  # 5: max-hold by the float compare instead of the key order
    def _fold(self, rows, spectra, first, op):
        out = np.array(rows, np.float32, copy=True)
        for u in range(spectra.shape[0]):
            r = (first + u) % out.shape[0]
            with np.errstate(invalid="ignore"):
                out[r] = spectra[u] if op == capi.BASELINE_SET else np.where(spectra[u] > out[r], spectra[u], out[r])
        return out


class KeepsStaleCounts(ModelPlan):  # 6: the units a smaller resubmit no longer has still count
    def _total(self, slot, counts):
        return int(counts.sum() + self.slot[slot].counts[len(counts):].sum())


class BufferIndexForTheEntry(ModelPlan):  # 7: an averaged plan's group g takes table entry first + g K
    def _entry(self, g):
        return g * self.average


class RefusalChangesState(ModelPlan):  # 8: a state change refused for a pending slot is made all the same
    def set_table(self, center_freqs):
        self._set_table(center_freqs)
        super().set_table(center_freqs)

    def set_floor_window(self, train, guard=0):
        self._set_floor_window(train, guard)
        super().set_floor_window(train, guard)

    def set_baseline(self, baseline):
        self._set_baseline(baseline)
        super().set_baseline(baseline)


# (the broken model; the plans it can differ on; the kinds of step at which the runner may first fail.  A wrong record shows at the
# collect that returns it -- or, behind a collect of the counts only, in that step's windows; a wrong row in the next read-back or the
# next collect; a refusal that changed the row count also in the status of the next indexed submit)
BROKEN = [
    (KeepsTheOldWindow, lambda p: p["detect"] == "window", {"collect", "counts"}),
    (NoneIsTheLastWindow, lambda p: p["detect"] == "window", {"collect", "counts"}),
    (RowIgnoresFirst, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline"}),
    (FoldsAnotherSlot, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline", "update_baseline"}),
    (MaxByFloatCompare, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline"}),
    (KeepsStaleCounts, lambda p: True, {"collect", "counts"}),
    (BufferIndexForTheEntry, lambda p: p["average"] > 1, {"collect", "counts"}),
    (RefusalChangesState, lambda p: True, {"collect", "counts", "get_baseline", "submit"}),
]


@pytest.mark.parametrize("broken,concerns,kinds", BROKEN, ids=[b[0].__name__ for b in BROKEN])
def test_the_runner_fails_against_a_broken_model(source, broken, concerns, kinds):
    failures = []
    for seed, index, sc in _scripts():
        if not concerns(sc["plan"]):
            continue
        try:
            sequence_run.run(sc, lambda d: broken(d, source(d)), source, seed, index)
        except sequence_run.SequenceFailure as e:
            assert isinstance(e.cause, AssertionError), e  # a difference the runner saw, not an accident
            assert f"seed {seed} script {index} step {e.step_index}" in str(e) and "script = {" in str(e)
            failures.append((seed, index, e.step_index, e.kind))
    print(broken.__name__, failures)
    assert failures, f"no committed script fails against {broken.__name__}: the slice cannot see that fault"
    assert {kind for _, _, _, kind in failures} <= kinds, failures
