"""The floor window (scn_plan_set_floor_window, scn_local_floor_from_spectrum) on a machine without a GPU: the host form of the
definition against the numpy restatement of tests/local_floor_ref.py, bit for bit; its rejections; and the equivalence the GPU's
kernel rests on -- counting the cells below a bin decides exactly what selecting the rank and adding the offset decides."""
import ctypes as C

import numpy as np
import pytest

from scanner_amd import capi
from tests import floor_ref, local_floor_ref
from tests.test_floor_cpu import _spectra

WINDOWS = ((1, 0), (16, 2), (128, 64))
PERMILLES = (capi.FLOOR_MIN, 0, 750, 1000)
SENTINEL = np.float32(-12345.5)


def _host(s, train, guard, **kw):
    """scn_local_floor_from_spectrum into a sentinel-filled array"""
    return capi.local_floor_from_spectrum(s, train, guard, out=np.full(s.size, SENTINEL, np.float32), **kw)


def _assert_same(got, want, what):
    """bit for bit on the evaluated bins (the reference holds NaN elsewhere), the sentinel untouched on the others"""
    ev = ~np.isnan(want)
    assert floor_ref.same_bits(got[ev], want[ev]), what
    assert np.all(got[~ev].view(np.uint32) == SENTINEL.view(np.uint32)), f"{what}: an entry of a bin the mask removes was written"


@pytest.mark.parametrize("n", [16, 17, 64, 1000, 4097, 65536])
def test_host_form_equals_the_reference(built_lib, n):
    L = capi.lib()
    spectra = _spectra(n)
    for train, guard in WINDOWS:
        if not local_floor_ref.valid(n, train, guard):  # the library agrees, and says why
            s = spectra["random"]
            out = np.zeros(n, np.float32)
            st = L.scn_local_floor_from_spectrum(s.ctypes.data_as(C.c_void_p), n, 0, 0.0, 0, train, guard, out.ctypes.data_as(C.c_void_p))
            assert st == capi.E_INVALID and b"no reference cell" in L.scn_last_error(), (n, train, guard)
            continue
        for name, s in spectra.items():
            ws = local_floor_ref.WindowSort(s, train, guard)
            for pm in PERMILLES:
                _assert_same(_host(s, train, guard, floor_permille=pm), ws.floors(pm), (n, train, guard, name, pm))
    assert local_floor_ref.valid(n, 1, 0) and (n < 1000 or local_floor_ref.valid(n, 128, 64))  # (the cases above did run)
    # the mask's parameters are the descriptor's: no DC mask, another band
    s = spectra["-inf among finite"]
    for dc, ub in ((0, 0.75), (2, 0.5), (4, 1.0)):
        for train, guard in WINDOWS:
            if local_floor_ref.valid(n, train, guard, ub, dc):
                _assert_same(_host(s, train, guard, dc_ignore_bins=dc, use_bandwidth=ub, floor_permille=750),
                             local_floor_ref.floors(s, train, guard, 750, ub, dc), (n, dc, ub, train, guard))


def test_cell_counts_are_the_definition_s(built_lib):
    """written out where the answer is known: n = 16 evaluates i in {2, 3, 4, 12, 13, 14}; interior bins have 2 train cells"""
    assert list(local_floor_ref.cell_counts(16, 1, 0)) == [1, 2, 1, 1, 2, 1]
    assert local_floor_ref.valid(16, 1, 0) and not local_floor_ref.valid(16, 1, 1)
    m = local_floor_ref.cell_counts(4096, 16, 2)
    assert m.max() == 32 and m.min() == 16 and np.count_nonzero(m == 32) > 2900  # the band's edges and the DC hole have fewer
    # permille 1000 is the window's maximum, FLOOR_MIN its minimum: on a ramp, the farthest cell above / below
    n = 64
    s = np.empty(n, np.float32)
    s[(np.arange(n) + n // 2) % n] = np.arange(n, dtype=np.float32)  # power_db = i
    hi, lo = _host(s, 2, 1, floor_permille=1000), _host(s, 2, 1, floor_permille=capi.FLOOR_MIN)
    for i in (20, 40):  # interior bins, away from the DC hole (29 ... 35) and the band's edges (8, 56)
        j = (i + n // 2) % n
        assert hi[j] == i + 3 and lo[j] == i - 3
    j = (8 + n // 2) % n  # the band's lower edge: the cells are 10 and 11 only
    assert hi[j] == 11 and lo[j] == 10
    j = (28 + n // 2) % n  # beside the DC hole: 25, 26 below; 30, 31 are masked and take up distance
    assert hi[j] == 26 and lo[j] == 25


def test_rejections(built_lib):
    L = capi.lib()
    s = np.zeros(64, np.float32)
    out = np.zeros(64, np.float32)
    sp, op = s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    f = L.scn_local_floor_from_spectrum
    assert f(sp, 64, 0, 0.0, 0, 0, 1, op) == capi.E_INVALID and b"train" in L.scn_last_error()   # train = 0 with a guard
    assert f(sp, 64, 0, 0.0, 0, 129, 0, op) == capi.E_INVALID and b"train" in L.scn_last_error()
    assert f(sp, 64, 0, 0.0, 0, 1, 65, op) == capi.E_INVALID and b"guard" in L.scn_last_error()
    assert f(sp, 16, 0, 0.0, 0, 1, 1, op) == capi.E_INVALID and b"i = 3" in L.scn_last_error()   # bin 3: i = 1 out of band, i = 5 in the DC mask
    assert f(sp, 16, 0, 0.0, 0, 1, 0, op) == capi.OK
    assert f(None, 64, 0, 0.0, 0, 4, 1, op) == capi.E_INVALID
    assert f(sp, 64, 0, 0.0, 0, 4, 1, None) == capi.E_INVALID
    assert f(sp, 0, 0, 0.0, 0, 4, 1, op) == capi.E_INVALID
    assert f(sp, 64, 0, 0.0, 1001, 4, 1, op) == capi.E_INVALID and b"floor_permille" in L.scn_last_error()
    assert f(sp, 64, 4, 0.01, 0, 4, 1, op) == capi.E_INVALID  # the band is the DC mask's bins: nothing is evaluated
    assert f(sp, 64, 0, 0.0, 0, 4, 1, op) == capi.OK
    # the setter refuses a null plan before it looks for a device
    assert L.scn_plan_set_floor_window(None, 16, 2) == capi.E_INVALID and b"null plan" in L.scn_last_error()


def test_no_window_is_the_unit_wide_floor(built_lib):
    s = _spectra(1000)["random"]
    got = _host(s, 0, 0, floor_permille=250)
    from tests import tolerances as tol

    ev = tol.evaluated_mask(1000)
    assert np.all(got[ev].view(np.uint32) == np.float32(floor_ref.floor_db(s, 250)).view(np.uint32)) and np.all(got[~ev] == SENTINEL)


@pytest.mark.parametrize("threshold", [0.0, 3.0, -2.5, 1e9, -1e9])
def test_counting_decides_what_selecting_decides(threshold):
    """hit iff power_db > fl(v_(r) + threshold)  <=>  #{cells c: fl(c + threshold) < power_db} >= r + 1 -- on every value pattern
    (ties, -0.0 / +0.0, -inf cells, all -inf), at an offset that absorbs every value (1e9) and at ordinary ones"""
    some = 0
    for n in (64, 1000, 4097):
        for name, s in _spectra(n).items():
            for train, guard in ((1, 0), (16, 2)):
                for pm in PERMILLES:
                    fl = local_floor_ref.floors(s, train, guard, pm)
                    i_sort, _ = local_floor_ref.hit_bins(s, fl, threshold)
                    i_count, _ = local_floor_ref.hit_bins_by_count(s, threshold, train, guard, pm)
                    assert np.array_equal(i_sort, i_count), (n, name, train, guard, pm)
                    some += i_sort.size
    assert some > 0  # (at 1e9 too: a floor of -inf keeps its cut at -inf, and every finite bin lies above it)
    allinf = np.full(64, -np.inf, np.float32)
    assert local_floor_ref.hit_bins_by_count(allinf, threshold, 4, 1)[0].size == 0  # a unit that is all -inf has no hits
