"""tests/sequence_cases.py's committed seed list on the CPU: it covers what it is there for, the runner (tests/sequence_run.py) passes
against the model (tests/sequence_model.py) for every committed script -- so the scripts are legal under the header's rules and the
checker agrees with itself --, and the runner FAILS against eighteen deliberately broken models, each at the kind of step its fault
must show at: the CPU-side proof that tests/test_plan_sequences_gpu.py would fail on the state faults it is there for."""
import functools
import hashlib
import time

import numpy as np
import pytest

from scanner_amd import capi
from tests import sequence_cases as cases
from tests import sequence_run, trace_ref
from tests.sequence_model import ModelPlan, numpy_source


@functools.lru_cache(maxsize=None)
def _scripts():
    return [(seed, index, sc) for seed in cases.SEEDS for index, sc in enumerate(cases.draw(seed))]


def test_draw_is_deterministic_and_made_of_literals():
    seed = cases.SEEDS[0]
    a, b = cases.draw(seed), cases.draw(seed)
    assert repr(a) == repr(b) and len(a) == cases.SCRIPTS_PER_SEED
    assert eval(repr(a), {}) == a, "a script must survive repr(): that is how a failure is pasted into a regression test"


# sha256 of repr(draw(seed)) as the generator gave it before it drew the history, the trace, the levels and the emitters
FIRST_PASS = {
    2414: "d237053b8e32831f5ae5c0890dc0aadd2bf415eacb73ba97da6bf599f45e9f68",
    2240: "982b43feae784e6f63d22416f147bc0ff55f30170d277b8b65709dbd36f9a377",
    488: "c233418ff7f8ebbcf457cdc806cde565aaab413a5b6bc3a27815546d16bebf48",
    119: "4fd97e29664bab8c7cb0475fd4e57d27fed4bea05dcc36e44ce0640b888f390e",
    386: "24ce5784736d219b78bc2fdfca2cf82ed3699d4f76ee8ebff55fd451dc017b1c",
    237: "42b353789d31b04e1e072bfe01fb838950c982d3ce25b28e91559a9d302cc54b",
    362: "ba64b51ff6f132fa7a79d7fe9fd30806f07e671cb7802e92bf3b246de9b4642c",
    280: "e8b89ea1a2a16250e5f859b3e883e0372482afef445947bed614bd0d13e2707e",
    49: "5d9ae64767479c6d86c92c5a26384b02f994818e882cd10959936bcb0a1a022a",
}


def test_the_second_pass_leaves_the_first_as_it_was():
    """with the steps of NEW_OPS stripped, every seed that was committed before them gives exactly the scripts it gave then"""
    for seed, digest in FIRST_PASS.items():
        assert seed in cases.SEEDS
        scripts = cases.draw(seed)
        assert hashlib.sha256(repr([cases.strip_new(sc) for sc in scripts]).encode()).hexdigest() == digest, seed
        assert any(st["op"] in cases.NEW_OPS for sc in scripts for st in sc["steps"]), seed


def test_the_committed_seeds_cover_what_they_are_there_for():
    got = cases.coverage([sc for _, _, sc in _scripts()])
    missing = cases.required() - got
    assert not missing, sorted(missing, key=str)
    # stated once more, without the helper: every (detector, size family) pair the header allows, each with its own plan
    pairs = {(sc["plan"]["detect"], cases.FAMILY_OF[sc["plan"]["n"]]) for _, _, sc in _scripts()}
    assert pairs == {(d, f) for d in cases.DETECTORS for f in cases.FAMILIES}
    refusals = sum(st["expect"] != capi.OK for _, _, sc in _scripts() for st in cases.strip_new(sc)["steps"])
    assert len(_scripts()) / 6 <= refusals <= len(_scripts()), (refusals, len(_scripts()))  # the first pass: about one per three scripts
    new = sum(st["expect"] != capi.OK for _, _, sc in _scripts() for st in sc["steps"] if st["op"] in cases.NEW_OPS)
    assert len(_scripts()) <= new <= 8 * len(_scripts()), (new, len(_scripts()))  # the second: a few per script


def test_the_limits_of_a_script():
    for seed, index, sc in _scripts():
        p = sc["plan"]
        assert p["max_batch"] // p["average"] <= cases.max_units(p["n"]) and p["max_batch"] % p["average"] == 0, (seed, index)
        assert p["average"] == 1 or p["n"] in cases.FAMILIES["averaged"], (seed, index)
        assert len(cases.strip_new(sc)["steps"]) <= 60, (seed, index)
        # (the second pass lays at most MAX_NEW_STEPS steps between them: folds, read-outs and pages, each a single small call)
        assert len(sc["steps"]) <= 60 + cases.MAX_NEW_STEPS and cases.MAX_NEW_STEPS == 45, (seed, index)


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
    assert min(stats[key] for key in ("history_words", "confirmed_records", "trace_cells", "level_counters", "emitter_records", "seam_emitters")) > 0


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


# -- the hit history, the sweep trace, the level histogram ---------------------------------------------------------------------------------
class FoldReadsTheLowestSlot(ModelPlan):  # 9: a trace or levels fold reads the lowest collected slot, not the one named
    def _source_slot(self, slot):
        return next(s for s in range(capi.NUM_SLOTS) if self.slot[s].last is not None)


class FoldKeepsTheOldUnitCount(ModelPlan):  # 10: a fold of a smaller resubmit folds the previous submit's unit count
    def _fold_count(self, s):
        return max(s.last["units"], s.units_before) if s.last["units"] else 0


class FoldTakesTheBufferIndex(ModelPlan):  # 11: an averaged indexed fold takes the centre of entry first + g K
    def _fold_entry(self, g):
        return g * self.average


class SameGeometryKeepsTheCells(ModelPlan):  # 12: set_trace or set_levels with the geometry it already has does not reset
    def _resets(self, old, new):
        return old != new


class LevelsOnTheTracesGrid(ModelPlan):  # 13: a levels fold uses the trace's f0 and cell_hz
    def _levels_grid(self):
        return (self.tr["f0"], self.tr["cell_hz"]) if self.tr is not None else super()._levels_grid()


class FoldsTwice(ModelPlan):  # 14: update_history is accepted twice for one submit
    def _already_folded(self, s):
        return False


class ConfirmsAStaleFold(ModelPlan):  # 15: collect_confirmed is accepted after another slot's fold
    def _is_latest(self, s):
        return s.folded != 0


class HistoryRowIgnoresFirst(ModelPlan):  # 16: the history row ignores first_index
    def _history_first(self, sub):
        return 0


class FoldsWithoutAList(ModelPlan):  # 17: a fold is accepted after set_table
    def _fold_list_ok(self, s):
        return s.pending is None and s.last is not None and bool(self.flags & capi.OUT_HITS)


class RefusedMergeIsMade(ModelPlan):  # 18: a refused merge_trace (the NaN window) has changed the trace
    def merge_trace(self, max_db, min_db, count, first=0):
        try:
            super().merge_trace(max_db, min_db, count, first)
        except capi.ScannerError:
            if self.tr is not None and first + len(count) <= self.tr["trace"][0].size:
                window = (np.nan_to_num(np.asarray(max_db, np.float32), nan=0.0), np.nan_to_num(np.asarray(min_db, np.float32), nan=0.0), np.asarray(count, np.uint64))
                self._merge(window, first)
            raise


def _can_trace(p):
    return bool(p["flags"] & capi.OUT_HITS) and (bool(p["flags"] & capi.OUT_SPECTRUM) or p["detect"] != "fixed")


def _has_hits(p):
    return bool(p["flags"] & capi.OUT_HITS)


# (the broken model; the plans it can differ on; the kinds of step at which the runner may first fail.  A wrong record shows at the
# collect that returns it -- or, behind a collect of the counts only, in that step's windows; a wrong row in the next read-back or the
# next collect; a refusal that changed the row count also in the status of the next indexed submit; a refused set_table that was made
# has dropped every list, which the next fold or confirmation of a collected slot answers with a refusal of its own)
BROKEN = [
    (KeepsTheOldWindow, lambda p: p["detect"] == "window", {"collect", "counts"}),
    (NoneIsTheLastWindow, lambda p: p["detect"] == "window", {"collect", "counts"}),
    (RowIgnoresFirst, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline"}),
    (FoldsAnotherSlot, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline", "update_baseline"}),
    (MaxByFloatCompare, lambda p: p["detect"] == "baseline", {"collect", "counts", "get_baseline"}),
    (KeepsStaleCounts, lambda p: True, {"collect", "counts"}),
    (BufferIndexForTheEntry, lambda p: p["average"] > 1, {"collect", "counts"}),
    (RefusalChangesState, lambda p: True, {"collect", "counts", "get_baseline", "submit", "update_history", "update_trace", "update_levels", "confirmed"}),
    # (the trace and the histogram are compared after every fold, merge and set: a wrong fold shows at the fold itself, a set that did
    # not reset at the set, a refused merge that was made at its refusal; a wrong row in the history at the fold, a refusal that was
    # accepted at the refusal)
    (FoldReadsTheLowestSlot, _can_trace, {"update_trace", "update_levels"}),
    (FoldKeepsTheOldUnitCount, _can_trace, {"update_trace", "update_levels"}),
    (FoldTakesTheBufferIndex, lambda p: _can_trace(p) and p["average"] > 1, {"update_trace", "update_levels"}),
    (SameGeometryKeepsTheCells, _can_trace, {"set_trace", "set_levels"}),
    (LevelsOnTheTracesGrid, _can_trace, {"update_levels"}),
    (FoldsTwice, _has_hits, {"refusal:update_history"}),
    (ConfirmsAStaleFold, _has_hits, {"refusal:confirmed"}),
    (HistoryRowIgnoresFirst, _has_hits, {"update_history"}),
    (FoldsWithoutAList, _has_hits, {"refusal:update_history", "refusal:update_trace", "refusal:update_levels"}),
    (RefusedMergeIsMade, _can_trace, {"refusal:merge_trace"}),
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
