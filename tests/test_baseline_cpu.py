"""The baseline detector (scn_plan_desc.detect = SCN_DETECT_BASELINE) on a machine without a GPU: tests/baseline_ref.py against the
definition written out as a double loop, its update against np.maximum and the key order, the checks scn_plan_create makes before
it looks for a device, the three entry points on a null plan, and the binding's constants against the header's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scanner_amd import capi
from tests import baseline_ref, floor_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scanner_hip.h")


def _scene(n, units, rows, seed):
    """spectra and a baseline that straddle each other, with the special values sprinkled over both"""
    rng = np.random.default_rng(seed)
    spectra = (rng.standard_normal((units, n)) * 3.0).astype(np.float32)
    baseline = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    for a in (spectra, baseline):
        flat = a.reshape(-1)
        pick = rng.choice(flat.size, max(4, flat.size // 16), replace=False)
        flat[pick] = rng.choice(np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32), pick.size)
    return spectra, baseline


@pytest.mark.parametrize("n", [16, 17, 1024])
def test_the_reference_equals_the_double_loop(n):
    units, rows = 5, 3
    spectra, baseline = _scene(n, units, rows, seed=n)
    some = 0
    for first in (0, 2, 7):
        for threshold in (0.0, 3.0, -1.5, np.float32(3e38), np.inf):
            fc = 100e6 + 6e6 * np.arange(units)
            seq = 1000 + 3 * np.arange(units, dtype=np.uint64)
            h, trig = baseline_ref.detect(spectra, baseline, first, threshold, fc, seq, 8000000, trigger_count=n // 8)
            want = baseline_ref.detect_brute(spectra, baseline, first, threshold)
            assert [(int(s), int(i)) for s, i in zip(h["seq_id"], h["i"])] == [(int(seq[u]), i) for u, i, j in want], (n, first, threshold)
            assert floor_ref.same_bits(h["power_db"], np.array([spectra[u, j] for u, i, j in want], np.float32))
            counts = np.bincount([u for u, i, j in want], minlength=units)
            assert np.array_equal(trig, counts > n // 8)
            for u in range(units):  # freq_hz is floor_ref's, per unit
                sel = h["seq_id"] == seq[u]
                assert np.array_equal(h["freq_hz"][sel], floor_ref._freq_hz(fc[u], h["i"][sel], n, 8000000))
            some += len(want)
    assert some > 0
    # the rules the header spells out, one row against one unit
    s = np.zeros((1, n), np.float32)
    for entry, hits in ((np.nan, False), (np.inf, False), (-np.inf, True), (-1.0, True), (0.0, False), (1.0, False)):
        got = baseline_ref.detect(s, np.full((1, n), entry, np.float32), 0, 0.0)[0]
        assert (len(got) == int(baseline_ref.evaluated(n).sum())) if hits else (len(got) == 0), entry
    minus_inf = np.full((1, n), -np.inf, np.float32)
    assert len(baseline_ref.detect(minus_inf, minus_inf, 0, 0.0)[0]) == 0  # a bin that is itself -inf is never a hit


def test_update_max_is_np_maximum_on_finite_data_and_the_key_order_elsewhere():
    rng = np.random.default_rng(3)
    base = (rng.standard_normal((4, 64)) * 5.0).astype(np.float32)
    spec = (rng.standard_normal((3, 64)) * 5.0).astype(np.float32)
    for first in (0, 2, 3):
        rows = baseline_ref.rows_of(first, 3, 4)
        got = baseline_ref.update(base, spec, first, capi.BASELINE_MAX)
        want = base.copy()
        want[rows] = np.maximum(base[rows], spec)
        assert floor_ref.same_bits(got, want), first
        got = baseline_ref.update(base, spec, first, capi.BASELINE_SET)
        want = base.copy()
        want[rows] = spec
        assert floor_ref.same_bits(got, want), first
        assert floor_ref.same_bits(baseline_ref.update(base, spec[:0], first, capi.BASELINE_MAX), base)  # no units: nothing changes
    # the key order: -inf < ... < -0.0 < +0.0 < ... < +inf, decided on the bits (np.maximum(-0.0, +0.0) may return either)
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32)
    a, b = np.meshgrid(vals, vals, indexing="ij")
    got = baseline_ref.update(a.reshape(1, -1), b.reshape(1, -1), 0, capi.BASELINE_MAX).reshape(a.shape)
    for x in range(vals.size):
        for y in range(vals.size):
            assert floor_ref.same_bits(got[x, y], vals[max(x, y)]), (vals[x], vals[y], got[x, y])
    # a learnt row starts at +inf and SET replaces it; MAX from +inf stays +inf
    inf_row = np.full((1, 6), np.inf, np.float32)
    assert floor_ref.same_bits(baseline_ref.update(inf_row, vals.reshape(1, -1), 0, capi.BASELINE_MAX), inf_row)
    assert floor_ref.same_bits(baseline_ref.update(inf_row, vals.reshape(1, -1), 0, capi.BASELINE_SET), vals.reshape(1, -1))


def _desc(**kw):
    d = capi.PlanDesc()
    d.struct_size = C.sizeof(capi.PlanDesc)
    d.n, d.sample_rate, d.sample_kind, d.enob, d.max_batch = 4096, 8000000, capi.KIND_SHORT_COMPLEX, 12, 16
    d.detect, d.flags = capi.DETECT_BASELINE, capi.OUT_HITS
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _create(d):
    L = capi.lib()
    h = C.c_void_p()
    st = L.scn_plan_create(C.byref(d), C.byref(h))
    if h:
        L.scn_plan_destroy(h)
    return st, L.scn_last_error()


def test_create_time_refusals_need_no_device(built_lib):
    # (flags = 0 asks for both outputs elsewhere; a baseline plan names SCN_OUT_HITS itself)
    for kw in (dict(flags=capi.OUT_SPECTRUM), dict(flags=0), dict(flags=capi.PLAN_OVERLAP_SLOTS), dict(mode=capi.MODE_TIME_DOMAIN),
               dict(mode=capi.MODE_TIME_DOMAIN, flags=capi.OUT_HITS),
               dict(flags=capi.OUT_SPECTRUM | capi.PLAN_OVERLAP_SLOTS), dict(detect=3), dict(detect=0xFFFFFFFF)):
        st, err = _create(_desc(**kw))
        assert st == capi.E_INVALID and b"detect" in err, (kw, st, err)


def test_valid_descriptors_reach_the_device_check(built_lib):
    """every valid combination passes the descriptor checks: without a GPU it fails on the device, never as SCN_E_INVALID"""
    import torch

    want = capi.OK if torch.cuda.is_available() else capi.E_NO_DEVICE
    for n in (16, 18, 64, 512, 1000, 1001, 4096, 8192, 16384, 32768, 65536):  # every route of scn_size_path
        for flags in (capi.OUT_HITS, capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS | capi.PLAN_OVERLAP_SLOTS):
            st, err = _create(_desc(n=n, flags=flags, max_batch=2))
            assert st == want, (n, flags, st, err)
    for n in (1024, 2048, 4096, 8192):  # averaged plans: a unit is a group
        for layout in (capi.AVG_DWELL, capi.AVG_SWEEPS):
            st, err = _create(_desc(n=n, average=2, average_layout=layout))
            assert st == want, (n, layout, st, err)
    st, err = _create(_desc(floor_permille=123456))  # floor_permille is ignored
    assert st == want, (st, err)


def test_the_entry_points_refuse_a_null_plan(built_lib):
    L = capi.lib()
    out = np.zeros(16, np.float32)
    assert L.scn_plan_set_baseline(None, 1, out.ctypes.data_as(C.c_void_p)) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_set_baseline(None, 0, None) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_update_baseline(None, 0, capi.BASELINE_MAX) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_get_baseline(None, 0, 1, out.ctypes.data_as(C.c_void_p)) == capi.E_INVALID and b"null plan" in L.scn_last_error()


def test_constants_follow_the_header():
    src = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(SCN_(?:DETECT|BASELINE)_[A-Z]+)\s*=\s*(\d+)", src))
    assert (capi.DETECT_FIXED, capi.DETECT_FLOOR, capi.DETECT_BASELINE) == (enum["SCN_DETECT_FIXED"], enum["SCN_DETECT_FLOOR"], enum["SCN_DETECT_BASELINE"])
    assert capi.DETECT_BASELINE == 2
    assert (capi.BASELINE_SET, capi.BASELINE_MAX) == (enum["SCN_BASELINE_SET"], enum["SCN_BASELINE_MAX"])
    assert capi.ABI_VERSION == int(re.search(r"#define\s+SCN_ABI_VERSION\s+(\d+)", src).group(1)) == 6  # additions only
    for name in ("scn_plan_set_baseline", "scn_plan_update_baseline", "scn_plan_get_baseline"):
        assert name in capi.SYMBOLS and re.search(r"\bSCN_API\b[^;{]*?\b%s\s*\(" % name, src), name
