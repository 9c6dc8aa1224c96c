"""Whole plan sequences on the GPU: every committed seed of tests/sequence_cases.py, scanner_amd.Plan run by tests/sequence_run.py
against the numpy model of tests/sequence_model.py.  What the per-feature files do not vary is what is varied here: the state one
submit inherits from the calls before it -- the floor window's table, the frequency table, the baseline's rows and their row count,
each slot's last spectrum, the two generations of hit regions, a smaller resubmit's counts -- over averaged and plain plans, every
detector, every wire format, up to four slots in flight, with the refusals the header names in between.  Between those steps lie the
folds, read-outs and pages of the four accumulators a plan keeps across submits -- the hit history with its confirmed lists, the sweep
trace with its emitters, the level histogram with its summary --, each fold reading what some earlier submit of some slot left: its
spectrum (the plan's or the caller's), its unit count, its centres or its run of the table, the history's epoch.

Every comparison is an equality on the plan's own stored spectrum (NaN positions compare as NaN): no guard band, no tolerance, no
exempt bin.  The spectrum itself is byte-identical to a twin's -- a fixed SCN_OUT_SPECTRUM-only plan with the same transform on the
same input, which also stands in for the spectrum a hits-only plan never returns -- and once per plan it is held at the suite's
usual bar (tolerances.compare_spectra) on ordinary units: against the oracle for K = 1, against the float64 mean power for K > 1.
tests/test_sequence_cases_cpu.py proves on the CPU that this runner fails on eighteen state faults; profiles/plan_sequences.md has the
times, the counts and three mutants of the library itself."""
import time

import numpy as np
import pytest

from scanner_amd import Plan, capi
from tests import sequence_cases as cases
from tests import sequence_run
from tests import tolerances as tol

pytestmark = pytest.mark.gpu

TOTAL = sequence_run.new_stats()
RAN = []


def _at_the_bar(oracle_mod):
    """once per plan: the stored spectrum of the ordinary units against the suite's references, at the suite's bar"""

    def check(d, raw, spectra, ordinary):
        n, k = d["n"], d["average"]
        if k == 1:
            o = oracle_mod.Oracle(n, cases.FS, 1e9, kind=d["kind"], enob=d["enob"], correct_dc=d["correct_dc"])
            want = o.run(np.ascontiguousarray(raw[ordinary]), want_hits=False, threads=8)[0]
        else:
            from tests.test_average_gpu import _ref64

            want = _ref64(oracle_mod, n, d["kind"], d["correct_dc"], raw, raw.shape[0] // k, k, d["layout"], d["enob"])[1][ordinary]
        tol.compare_spectra(spectra[ordinary], want)

    return check


def _run(script, oracle_mod, seed=None, index=None, stats=None):
    return sequence_run.run(script, lambda d: Plan(**sequence_run.plan_kwargs(d)), sequence_run.twin_source(), seed, index, stats,
                            check_spectrum=_at_the_bar(oracle_mod))


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_a_seed_of_plan_sequences(built_lib, oracle_mod, seed):
    stats = sequence_run.new_stats()
    t0 = time.perf_counter()
    for index, script in enumerate(cases.draw(seed)):
        _run(script, oracle_mod, seed, index, stats)
    print(f"seed {seed}: {time.perf_counter() - t0:.2f} s; {stats}")
    for key, value in stats.items():
        TOTAL[key] += value
    RAN.append(seed)


def _empty_submit(n, detect, nb_first):
    """a hits-only plan behind whose transform a detect kernel runs: an empty submit beside (and before, or after) a full one"""
    plan = dict(n=n, kind=capi.KIND_SHORT_COMPLEX, enob=14, correct_dc=True, use_bandwidth=0.75, dc_ignore_bins=4, trigger_count=1047, max_batch=4,
                max_hits=0, flags=capi.OUT_HITS, overlap=False, detect=detect, permille=0, average=1, layout=capi.AVG_DWELL, threshold=1.0)
    submit = dict(op="submit", expect=0, pinned=True, indexed=False, first_index=0, fc0=100e6, seq0=None, specials={})
    post = [("more", 0.0, 0.5), ("signals", 0, 0.0, 0.21), ("view",)] + ([("floor",)] if detect == "floor" else [])
    steps = [dict(op="set_baseline", expect=0, rows=1, seed=285153320)] if detect == "baseline" else []
    steps += [dict(submit, slot=1, units=nb_first, nb=nb_first, seed=1), dict(submit, slot=0, units=4 - nb_first, nb=4 - nb_first, seed=2),
              dict(op="collect", expect=0, slot=0, post=post), dict(op="collect", expect=0, slot=1, post=post)]
    return dict(plan=plan, steps=steps)


@pytest.mark.parametrize("nb_first", [0, 4])
@pytest.mark.parametrize("detect", ["floor", "baseline"])
@pytest.mark.parametrize("n", [512, 1000, 1001, 2048])
def test_an_empty_submit_on_a_hits_only_detector_plan(built_lib, oracle_mod, n, detect, nb_first):
    """Found by seed 2414, script 0, step 4: scn_submit with n_buffers = 0 on a hits-only baseline plan of 512 points returned
    SCN_E_HIP.  Such a plan's transform stores the spectrum into a buffer of the plan's own, which an empty submit never allocates, and
    the fused launchers (powers of two and mixed radix) refused a launch that named neither hits nor a spectrum before they looked at
    its size; Bluestein, the four-step pair and the averaged kernels looked at the size first.  An empty submit now launches nothing."""
    _run(_empty_submit(n, detect, nb_first), oracle_mod)


def test_every_comparison_was_an_equality(built_lib):
    """after the seeds: nothing was exempt, nothing had a tolerance but the one spectrum check per plan, and everything was compared"""
    if set(RAN) != set(cases.SEEDS):
        pytest.fail(f"the seeded cases did not all run and pass before this one: {sorted(RAN)}")
    print(TOTAL)
    assert TOTAL["exempt_records"] == 0 and TOTAL["tolerances"] == 0
    assert TOTAL["scripts"] == len(cases.SEEDS) * cases.SCRIPTS_PER_SEED == TOTAL["bar_checks"]
    assert min(TOTAL[key] for key in ("steps", "refusals", "spectrum_floats", "records", "windows", "window_records", "signals", "floors",
                                      "baseline_floats", "special_units")) > 0
    assert min(TOTAL[key] for key in ("history_words", "confirmed_records", "trace_cells", "level_counters", "emitter_records", "seam_emitters",
                                      "caller_buffer_folds")) > 0
