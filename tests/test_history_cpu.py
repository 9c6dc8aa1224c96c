"""The hit history's host forms (scn_history_fold_hits, scn_confirm_hits, through ctypes) held to tests/history_ref.py, the numpy
model written from the definition: seeded random hit lists folded forty times in a row -- bits fall off the top of the word --,
every refusal, and hand-written known answers.  Needs no device."""
import numpy as np
import pytest

from scanner_amd import capi
from tests import history_ref

MW = [(1, 1), (2, 2), (3, 5), (32, 32), (1, 32)]


def _hit_list(rng, n, n_units, ids, density):
    """an ordered hit list: per unit a random set of bins (none at all for some units), increasing i"""
    parts = []
    for u in range(n_units):
        if rng.random() < 0.25:
            continue  # an empty unit
        i = np.flatnonzero(rng.random(n) < density).astype(np.uint32)
        h = np.zeros(i.size, capi.HIT_DTYPE)
        h["seq_id"], h["i"] = ids[u], i
        h["power_db"] = rng.standard_normal(i.size).astype(np.float32)
        h["freq_hz"] = rng.integers(0, 1 << 40, i.size, dtype=np.uint64)
        parts.append(h)
    return np.concatenate(parts) if parts else np.zeros(0, capi.HIT_DTYPE)


@pytest.mark.parametrize("given_ids", [False, True])
@pytest.mark.parametrize("rows,first", [(1, 0), (5, 0), (5, 3), (5, 13)])
@pytest.mark.parametrize("n", [16, 100, 4096])
def test_host_forms_against_the_model(built_lib, n, rows, first, given_ids):
    rng = np.random.default_rng(1000 * n + 10 * rows + first + given_ids)
    hist, visits = history_ref.new(rows, n)
    want_hist, want_visits = hist.copy(), visits.copy()
    top_seen = False
    for sweep in range(40):
        n_units = int(rng.integers(0, rows + 1)) if sweep % 8 == 7 else rows  # (35 whole sweeps: every row passes 32 visits)
        ids = (7 + 3 * np.arange(n_units, dtype=np.uint64) + np.uint64(100 * sweep)) if given_ids else None
        hits = _hit_list(rng, n, n_units, history_ref.unit_ids(n_units, ids), density=(0.0, 0.5, 1.0, 0.1, 0.5)[sweep % 5])
        capi.history_fold_hits(hist, visits, hits, n_units, first=first, unit_seq_ids=ids)
        want_hist, want_visits = history_ref.fold(want_hist, want_visits, hits, n_units, first=first, seq_ids=ids)
        assert np.array_equal(hist, want_hist) and np.array_equal(visits, want_visits), sweep
        top_seen = top_seen or bool((hist >> 31).any())
        for m, window in MW:
            got = capi.confirm_hits(hist, hits, n_units, m, window, first=first, unit_seq_ids=ids)
            want = history_ref.confirm(want_hist, hits, n_units, m, window, first=first, seq_ids=ids)
            assert got.tobytes() == want.tobytes(), (sweep, m, window)
        assert capi.confirm_hits(hist, hits, n_units, 1, 1, first=first, unit_seq_ids=ids).tobytes() == hits.tobytes()
    assert visits.min() >= 33 and top_seen  # bits have reached the top of the word and fallen off it


def _hits(seq_i):
    h = np.zeros(len(seq_i), capi.HIT_DTYPE)
    for k, (seq, i) in enumerate(seq_i):
        h[k] = (seq, i, 1.5 + k, 1000 + k)
    return h


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.ScannerError as e:
        return e.status
    return capi.OK


def test_refusals(built_lib):
    n, rows = 16, 3
    hist, visits = history_ref.new(rows, n)
    hist[:] = 0x12345678
    before = hist.copy()
    # records left over: a seq_id no unit has, a unit's records out of order behind another's
    assert _status(capi.history_fold_hits, hist, visits, _hits([(0, 1), (5, 2)]), 2) == capi.E_INVALID
    assert _status(capi.history_fold_hits, hist, visits, _hits([(1, 1), (0, 2)]), 2) == capi.E_INVALID
    assert _status(capi.history_fold_hits, hist, visits, _hits([(0, 1)]), 0) == capi.E_INVALID
    assert _status(capi.confirm_hits, hist, _hits([(0, 1), (5, 2)]), 2, 1, 1) == capi.E_INVALID
    # i >= n
    assert _status(capi.history_fold_hits, hist, visits, _hits([(0, 1), (1, n)]), 2) == capi.E_INVALID
    assert _status(capi.confirm_hits, hist, _hits([(0, n)]), 1, 1, 1) == capi.E_INVALID
    # more units than rows: a row would be visited twice
    assert _status(capi.history_fold_hits, hist, visits, _hits([(0, 1)]), rows + 1) == capi.E_INVALID
    # m = 0, m > window, window = 33
    for m, window in ((0, 1), (0, 0), (3, 2), (1, 33), (33, 33)):
        assert _status(capi.confirm_hits, hist, _hits([(0, 1)]), 1, m, window) == capi.E_INVALID, (m, window)
    assert np.array_equal(hist, before) and not visits.any()  # a refused call changes nothing
    assert _status(capi.history_fold_hits, hist, visits, _hits([(0, 1), (1, n - 1)]), 2) == capi.OK


def test_known_answers(built_lib):
    """one bin hit on visits 1, 3 and 4 of five: confirmed at (3, 5) from visit 4 on, and not at (2, 2) on visit 3"""
    n, i = 16, 5
    hist, visits = history_ref.new(1, n)
    words = []
    for visit in range(1, 6):
        hits = _hits([(0, i)] if visit in (1, 3, 4) else [])
        capi.history_fold_hits(hist, visits, hits, 1)
        words.append(int(hist[0, i]))
        if visit == 3:
            assert len(capi.confirm_hits(hist, hits, 1, 2, 2)) == 0 and len(capi.confirm_hits(hist, hits, 1, 2, 3)) == 1
            assert len(capi.confirm_hits(hist, hits, 1, 3, 5)) == 0
        if visit == 4:
            assert capi.confirm_hits(hist, hits, 1, 3, 5).tobytes() == hits.tobytes()
            assert capi.confirm_hits(hist, hits, 1, 2, 2).tobytes() == hits.tobytes()
    assert words == [0b1, 0b10, 0b101, 0b1011, 0b10110] and visits[0] == 5
    assert not np.delete(hist[0], i).any()
    # a record of the fifth visit's list would be held against 0b10110: three of five, but not the last
    probe = _hits([(0, i)])
    assert len(capi.confirm_hits(hist, probe, 1, 3, 5)) == 1 and len(capi.confirm_hits(hist, probe, 1, 1, 1)) == 0
    # at (1, 1) the output is the input: every record of a list was folded in as a hit
    hist2, visits2 = history_ref.new(4, n)
    full = _hits([(9, 0), (9, 7), (9, 15), (2, 3), (4, 4), (4, 5)])
    ids = np.array([9, 2, 77, 4], np.uint64)
    capi.history_fold_hits(hist2, visits2, full, 4, first=2, unit_seq_ids=ids)
    assert capi.confirm_hits(hist2, full, 4, 1, 1, first=2, unit_seq_ids=ids).tobytes() == full.tobytes()
    assert np.array_equal(np.flatnonzero(hist2[2]), [0, 7, 15]) and np.array_equal(np.flatnonzero(hist2[3]), [3])
    assert not hist2[0].any() and np.array_equal(np.flatnonzero(hist2[1]), [4, 5]) and visits2.tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_half_density_sweeps_confirm_about_half(built_lib, seed):
    """what tests/test_history_gpu.py asks of its floor-plan scenes, on synthetic lists: independent half-density sweeps leave a
    (2, 2) list that is neither empty nor the full list -- between 10 % and 90 % of it -- from the third sweep on"""
    n, units = 128, 3
    rng = np.random.default_rng(seed)
    hist, visits = history_ref.new(5, n)
    for sweep in range(6):
        parts = []
        for u in range(units):
            i = np.flatnonzero(rng.random(n) < 0.5)
            parts += [(u, int(x)) for x in i]
        hits = _hits(parts)
        capi.history_fold_hits(hist, visits, hits, units)
        if sweep >= 2:
            got = len(capi.confirm_hits(hist, hits, units, 2, 2))
            assert 0.1 * len(hits) <= got <= 0.9 * len(hits), (sweep, got, len(hits))
