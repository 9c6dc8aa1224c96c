"""tests/detector_cases.py held to the launchers it was read from, and the conditions tests/test_detector_geometry_gpu.py relies on
that the mask and the window alone decide -- all without a GPU.

Each `*_instance` function restates a launcher's chain of `if (n <= ...) return launch<...>`.  The tests below find every step in the
launcher's own body and fail, naming detector_cases.py, when a step has moved, gone or been added: the GPU cases were chosen by the
instantiation they reach, and a moved step would silently take them off it."""
import os

import numpy as np
import pytest

from tests import detector_cases as dc
from tests import local_floor_ref
from tests import tolerances as tol
from tests.test_launch_caps_cpu import CSRC, _body


def _reads(body, expr, what, fname):
    assert expr in body, f"{fname}: {what} no longer reads `{expr}` -- restate it in tests/detector_cases.py (and in this test)"


def _targs(inst):
    return ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in inst)


def _chain(fname, signature, var, steps, last, what):
    body = _body(fname, signature)
    for top, inst in steps:
        _reads(body, f"if ({var} <= {top}u) return launch<{_targs(inst)}>(a, num_cus, stream);", f"{what}'s step at {top}", fname)
    _reads(body, f"  return launch<{_targs(last)}>(a, num_cus, stream);", f"{what}'s last step", fname)
    assert body.count("return launch<") == len(steps) + 1, f"{fname}: {what} has another number of steps -- tests/detector_cases.py"
    return body


def test_local_floor_launcher():
    f = "scn_floor_local.hip"
    _chain(f, "hipError_t scn_launch_floor_local(", "n", dc.LOCAL_FLOOR_STEPS, dc.LOCAL_FLOOR_LAST, "the window launcher")
    with open(os.path.join(CSRC, f)) as fh:
        src = fh.read()
    _reads(src, "static constexpr uint32_t CAP = 4u * (uint32_t)T * (uint32_t)RUNS;", "the tile", f)
    _reads(src, "for (uint32_t tile0 = 0; tile0 < n; tile0 += G::CAP) {", "the tile loop", f)
    assert [dc.local_floor_instance(n) for n in (16, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 65536)] == [
        (64, 1), (64, 1), (64, 2), (64, 2), (256, 1), (256, 1), (256, 4), (256, 4), (1024, 2), (1024, 2), (1024, 4), (1024, 4)]
    # one tile up to 16384 points; 20000: two, the second holding 3616 bins; 32768: two full ones; 65535: four, the last one bin short
    assert [dc.local_floor_tiles(n) for n in (16384, 20000, 32768, 65535, 65536)] == [
        (1, 16384), (2, 3616), (2, 16384), (4, 16383), (4, 16384)]
    assert dc.local_floor_tiles(301) == (1, 301) and dc.local_floor_tiles(4097) == (1, 4097)


def test_floor_launcher():
    f = "scn_floor.hip"
    _chain(f, "hipError_t scn_launch_floor(", "n", dc.FLOOR_STEPS, dc.FLOOR_LAST, "the floor launcher")
    kernel = _body(f, "__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_floor_kernel(")
    _reads(kernel, "const uint32_t trips = REREAD ? (n + T - 1u) / T : (uint32_t)KPT;", "the re-read route's trips", f)
    assert [dc.floor_instance(n) for n in (16, 128, 129, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 65536)] == [
        (64, 2, False), (64, 2, False), (64, 8, False), (64, 8, False), (256, 4, False), (256, 4, False), (256, 16, False), (256, 16, False),
        (1024, 8, False), (1024, 8, False), (1024, 16, False), (1024, 16, False), (1024, 1, True), (1024, 1, True)]
    # 20000: 20 trips, 544 threads of the last hold a bin; 65535: the last trip one thread short; 32768 and 65536: full trips
    assert [dc.floor_reread_trips(n) for n in (20000, 32768, 65535, 65536)] == [(20, 544), (32, 1024), (64, 1023), (64, 1024)]


def test_baseline_launcher():
    f = "scn_baseline.hip"
    size = _body(f, "hipError_t launch_size(")
    for top, team in dc.BASELINE_TEAM_STEPS:
        _reads(size, f"if (a.n <= {top}u) return launch_team<{team}, VEC>(a, num_cus, stream);", f"the team's step at {top}", f)
    _reads(size, f"  return launch_team<{dc.BASELINE_TEAM_LAST}, VEC>(a, num_cus, stream);", "the team's last step", f)
    assert size.count("return launch_team<") == len(dc.BASELINE_TEAM_STEPS) + 1, f"{f}: another number of team steps -- tests/detector_cases.py"
    team = _body(f, "hipError_t launch_team(")
    _reads(team, "const uint32_t per_trip = (uint32_t)T * (VEC ? 4u : 1u), trips = (a.n + per_trip - 1u) / per_trip;", "the trips", f)
    _reads(team, "if (trips <= 1u) return launch<T, VEC, 1>(a, num_cus, stream);", "U = 1", f)
    _reads(team, "if (trips <= 2u) return launch<T, VEC, 2>(a, num_cus, stream);", "U = 2", f)
    _reads(team, "  return launch<T, VEC, 4>(a, num_cus, stream);", "U = 4", f)
    assert team.count("return launch<") == 3, f"{f}: another number of U steps -- tests/detector_cases.py"
    top = _body(f, "hipError_t scn_launch_baseline_detect(")
    _reads(top, "const bool vec = a.n % 4u == 0 && (((uintptr_t)a.power_db | (uintptr_t)a.baseline_db) & 15u) == 0;", "the choice of the 16-byte loads", f)
    _reads(top, "return vec ? launch_size<true>(a, num_cus, stream) : launch_size<false>(a, num_cus, stream);", "its use", f)
    kernel = _body(f, "__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_baseline_kernel(")
    _reads(kernel, "for (uint32_t k0 = 0; k0 < trips; k0 += (uint32_t)U) {", "the kernel's loop", f)
    # the kernel's own header comment, size by size, and the four the issue names
    assert [dc.baseline_instance(n) for n in (16, 256, 512, 1000, 1024, 2048, 4096, 8192, 16384, 65536)] == [
        (64, True, 1), (64, True, 1), (64, True, 2), (256, True, 1), (256, True, 1), (256, True, 2), (256, True, 4), (1024, True, 2),
        (1024, True, 4), (1024, True, 4)]
    assert [dc.baseline_instance(n) for n in (18, 64, 90, 301, 501, 1001, 4097, 65535)] == [
        (64, False, 1), (64, True, 1), (64, False, 2), (64, False, 4), (64, False, 4), (256, False, 4), (1024, False, 4), (1024, False, 4)]
    assert dc.baseline_instance(4096, aligned=False) == (256, False, 4)
    assert dc.baseline_loop_trips(501) == 2 and dc.baseline_loop_trips(301) == 2 and dc.baseline_loop_trips(65536) == 4
    assert dc.baseline_loop_trips(65535) == 16 and dc.baseline_loop_trips(90) == 1


def test_the_cases_reach_every_reachable_instantiation():
    """Window and floor: every step of the chain is a range of sizes a plan takes, so every instantiation is reachable, and reached.
    Baseline: 18 instantiations are compiled (T x VEC x U), 12 are reachable.  T = 64 serves n <= 512: with 16-byte loads that is at
    most 2 trips of 256 bins, so <64, VEC, 4> is not; T = 256 serves 513 ... 4096: with 4-byte loads at least 3 trips of 256 bins, so
    <256, scalar, 1> and <256, scalar, 2> are not; T = 1024 serves n > 4096: at least 2 trips of 4096 bins and at least 5 of 1024, so
    <1024, VEC, 1>, <1024, scalar, 1> and <1024, scalar, 2> are not.  An n % 4 == 0 on the 4-byte loads needs a spectrum or a baseline
    that is not 16-byte aligned, which no device allocation is: it reaches nothing the odd sizes do not."""
    window_sizes = dc.SWEEP_SIZES + dc.RESIDUE_SIZES
    assert {dc.local_floor_instance(n) for n in window_sizes} == dc.reachable(dc.local_floor_instance) == {i for _, i in dc.LOCAL_FLOOR_STEPS} | {dc.LOCAL_FLOOR_LAST}
    unit_sizes = dc.EDGE_SIZES + dc.MASK_SIZES
    assert {dc.floor_instance(n) for n in unit_sizes} == dc.reachable(dc.floor_instance) == {i for _, i in dc.FLOOR_STEPS} | {dc.FLOOR_LAST}
    want = {(64, True, 1), (64, True, 2), (64, False, 1), (64, False, 2), (64, False, 4), (256, True, 1), (256, True, 2), (256, True, 4),
            (256, False, 4), (1024, True, 2), (1024, True, 4), (1024, False, 4)}
    assert dc.reachable(dc.baseline_instance) == want
    assert dc.reachable(dc.baseline_instance, aligned=False) <= want
    # (64, scalar, 1) needs an n <= 64 that is no multiple of 4: tests/test_baseline_gpu.py's 18 is that one; the rest is reached here
    # and <256, VEC, 1> an n % 4 == 0 in 516 ... 1024: the averaged baseline case
    assert {dc.baseline_instance(n) for n in unit_sizes + [dc.AVERAGE_DETECTOR_SIZES["baseline"]]} == want - {(64, False, 1)}
    assert dc.baseline_instance(18) == (64, False, 1)
    # what the issue's list says each edge size is there for
    assert dc.baseline_instance(501) == (64, False, 4) and dc.baseline_instance(2048) == (256, True, 2)
    assert dc.baseline_instance(4097) == (1024, False, 4) and dc.local_floor_instance(4097) == (1024, 2)
    assert dc.floor_instance(20000) == (1024, 1, True) and dc.floor_reread_trips(20000)[1] < 1024 and dc.local_floor_tiles(20000)[0] == 2
    assert [dc.local_floor_instance(n) for n in dc.SWEEP_SIZES] == [(64, 1), (256, 1)]
    assert [dc.local_floor_instance(n) for n in dc.RESIDUE_SIZES] == [(64, 2), (64, 2), (256, 4), (1024, 2)] + [(1024, 4)] * 4


def test_the_matrix_is_the_one_stated():
    assert dc.MASKS == [(0.75, 4), (1.0, 0), (0.5, 8), (0.9, 1), (1.0, 4)]
    assert len(dc.SWEEP) == 132 == len(set(dc.SWEEP)) and {(t, g) for t in range(1, 13) for g in range(10)} <= set(dc.SWEEP)
    assert len(dc.RESIDUES) == 22 == len(set(dc.RESIDUES)) and len(dc.RESIDUES_EXTRA) == 6
    pairs = {(g % 4, t % 4) for t, g in dc.RESIDUES[:16]}
    assert pairs == {(a, b) for a in range(4) for b in range(4)}, "RESIDUES misses a pair (guard mod 4, train mod 4)"
    # the windows the kernel's chunk arithmetic splits on: guard <= 2 and above, each guard mod 4, an odd train above 1
    assert {g % 4 for t, g in dc.SWEEP if 3 <= g <= 63} == {0, 1, 2, 3} and any(t % 2 and t > 1 for t, g in dc.SWEEP)
    assert dc.EDGE_SIZES == [90, 301, 501, 2048, 3000, 4097, 10000, 20000, 32768, 65535]
    assert {16, 64, 1001, 4096, 8192, 65536} <= set(dc.MASK_SIZES)
    # natural bin 4096 of 4097 points -- all the last trip of the baseline's <1024, scalar, 4> holds -- is a bin under the full mask only
    assert dc.EXTRA_UNIT_CASES == [(4097, dc.FULL_MASK)] and dc.baseline_loop_trips(4097) == 2
    assert not tol.evaluated_mask(4097, *dc.DEFAULT_MASK)[4096] and tol.evaluated_mask(4097, *dc.FULL_MASK)[4096]
    assert all(2 <= dc.units_for(n) <= 5 for n in dc.EDGE_SIZES + dc.MASK_SIZES + dc.RESIDUE_SIZES + dc.SWEEP_SIZES)


@pytest.mark.parametrize("n", dc.SWEEP_SIZES)
@pytest.mark.parametrize("mask", [dc.DEFAULT_MASK, dc.FULL_MASK])
def test_sweep_validity(n, mask):
    """the invalid share of the sweep is exactly the one stated: the GPU sweep cannot hollow out into refusals"""
    invalid = [w for w in dc.SWEEP if not local_floor_ref.valid(n, *w, *mask)]
    assert sorted(invalid) == sorted(dc.SWEEP_INVALID[(n, mask)]), (n, mask, invalid)
    assert len(dc.SWEEP) - len(invalid) >= 129


@pytest.mark.parametrize("n", dc.RESIDUE_SIZES)
@pytest.mark.parametrize("mask", [dc.DEFAULT_MASK, dc.FULL_MASK])
def test_residues_are_valid(n, mask):
    ev = tol.evaluated_mask(n, *mask)[(np.arange(n) + n // 2) % n].astype(np.int64)  # by fftshift index
    c = np.concatenate([[0], np.cumsum(ev)])
    i = np.flatnonzero(ev)

    def count(lo, hi):  # evaluated bins with lo <= i' <= hi, clipped to the band: no wrap
        return c[np.clip(hi + 1, 0, n)] - c[np.clip(lo, 0, n)]

    for train, guard in dc.RESIDUES:
        m = count(i - guard - train, i - guard - 1) + count(i + guard + 1, i + guard + train)
        assert m.min() >= 1, (n, mask, train, guard)
        if n <= 4096:  # the prefix counts above against the reference's own
            assert np.array_equal(m, local_floor_ref.cell_counts(n, train, guard, *mask))
            assert local_floor_ref.valid(n, train, guard, *mask)


def test_masks_the_sizes_admit():
    """(0.5, 8) leaves no bin at 16 points -- the one (size, mask) a floor plan refuses; every other pair keeps some, and the full
    mask keeps all n"""
    empty = [(n, m) for n in dc.MASK_SIZES for m in dc.OTHER_MASKS if not tol.evaluated_mask(n, *m).any()]
    assert empty == [(16, (0.5, 8))]
    for n in dc.MASK_SIZES + dc.SIGNAL_SIZES + dc.RESIDUE_SIZES + dc.SWEEP_SIZES:
        assert tol.evaluated_mask(n, *dc.FULL_MASK).all(), n
    for n in dc.AVERAGE_SIZES:
        assert [int(tol.evaluated_mask(n, *m).sum()) for m in dc.AVERAGE_MASKS] == [n, n // 2 + 1 - 15, 2 * int(0.9 * n / 2.0) + 1 - 1]
