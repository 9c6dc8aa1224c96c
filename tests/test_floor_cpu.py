"""The floor detector (scn_plan_desc.detect / floor_permille, scn_floor_from_spectrum) on a machine without a GPU: the
descriptor's layout, the checks scn_plan_create makes before it looks for a device, and the host form of the definition
against the numpy restatement of tests/floor_ref.py, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scanner_amd import capi
from tests import floor_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_desc_layout(tmp_path):
    assert capi.ABI_VERSION == 6
    assert C.sizeof(capi.PlanDesc) == 88  # unchanged: the two fields came out of the reserved words, one of which remains
    assert capi.PlanDesc.detect.offset == 76 and capi.PlanDesc.floor_permille.offset == 80 and capi.PlanDesc.reserved.offset == 84
    f = tmp_path / "t.c"
    f.write_text('#include "scanner_hip.h"\n#include <stddef.h>\nint main(void){ return (int)(sizeof(scn_plan_desc) != 88) + '
                 '(int)(offsetof(scn_plan_desc, detect) != %d) + (int)(offsetof(scn_plan_desc, floor_permille) != %d) + '
                 '(int)(offsetof(scn_plan_desc, reserved) != %d) + (int)(sizeof(((scn_plan_desc *)0)->reserved) != 4) + '
                 '(int)(SCN_ABI_VERSION != 6) + (int)(SCN_DETECT_FIXED != %d) + (int)(SCN_DETECT_FLOOR != %d) + '
                 '(int)(SCN_FLOOR_MIN != %du); }\n'
                 % (capi.PlanDesc.detect.offset, capi.PlanDesc.floor_permille.offset, capi.PlanDesc.reserved.offset,
                    capi.DETECT_FIXED, capi.DETECT_FLOOR, capi.FLOOR_MIN))
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0, "scn_plan_desc differs between the header and the ctypes binding"


def _desc(**kw):
    d = capi.PlanDesc()
    d.struct_size = C.sizeof(capi.PlanDesc)
    d.n, d.sample_rate, d.sample_kind, d.enob, d.max_batch = 4096, 8000000, capi.KIND_SHORT_COMPLEX, 12, 16
    d.detect = capi.DETECT_FLOOR
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


def test_invalid_floor_descriptors(built_lib):
    cases = [
        (dict(mode=capi.MODE_TIME_DOMAIN), b"detect"),
        (dict(flags=capi.OUT_SPECTRUM), b"detect"),
        (dict(detect=2), b"detect"),
        (dict(detect=0xFFFFFFFF), b"detect"),
        (dict(detect=2, mode=capi.MODE_TIME_DOMAIN), b"detect"),
        (dict(floor_permille=1001), b"floor_permille"),
        (dict(floor_permille=0xFFFFFFFE), b"floor_permille"),
        (dict(floor_permille=1 << 20), b"floor_permille"),
        # the band is the DC mask's bins: no bin is evaluated, so no rank exists (M - 1 would wrap)
        (dict(n=64, use_bandwidth=0.01), b"detect"),
        (dict(n=4096, use_bandwidth=0.001, dc_ignore_bins=8), b"detect"),
    ]
    for kw, msg in cases:
        st, err = _create(_desc(**kw))
        assert st == capi.E_INVALID and msg in err, (kw, st, err)


def test_valid_floor_descriptors_reach_the_device_check(built_lib):
    """Every valid combination passes the descriptor checks: without a GPU it fails on the device (SCN_E_NO_DEVICE), never
    as SCN_E_INVALID; with one the plan is made."""
    import torch

    want = capi.OK if torch.cuda.is_available() else capi.E_NO_DEVICE
    for n in (16, 64, 512, 1000, 1001, 4096, 8192, 16384, 32768, 65536):  # every route of scn_size_path
        for flags in (capi.OUT_HITS, capi.OUT_SPECTRUM | capi.OUT_HITS, 0, capi.OUT_HITS | capi.PLAN_OVERLAP_SLOTS):
            st, err = _create(_desc(n=n, flags=flags, max_batch=2))
            assert st == want, (n, flags, st, err)
    for pm in (0, 1, 250, 500, 999, 1000, capi.FLOOR_MIN):
        st, err = _create(_desc(floor_permille=pm))
        assert st == want, (pm, st, err)
    for n in (1024, 2048, 4096, 8192):  # with average > 1
        for layout in (capi.AVG_DWELL, capi.AVG_SWEEPS):
            st, err = _create(_desc(n=n, average=2, average_layout=layout))
            assert st == want, (n, layout, st, err)
    # floor_permille is read in floor mode only: a fixed plan ignores whatever it holds
    st, err = _create(_desc(detect=capi.DETECT_FIXED, floor_permille=123456))
    assert st == want, (st, err)


PERMILLES = (0, 1, 250, 500, 999, 1000, capi.FLOOR_MIN)


def _spectra(n):
    """name -> float32 [n]: the value patterns the definition has corners for"""
    rng = np.random.default_rng(n)
    out = {
        "random": (rng.standard_normal(n) * 7.0 - 4.0).astype(np.float32),
        "straddling 0 dB": (rng.standard_normal(n) * 1e-3).astype(np.float32),
        "three values": rng.choice(np.array([-3.25, 0.5, 17.0], np.float32), n),
        "all -inf": np.full(n, -np.inf, np.float32),
        "-0.0 and +0.0": rng.choice(np.array([-0.0, 0.0], np.float32), n),
        "-inf among finite": np.where(rng.random(n) < 0.4, -np.inf, rng.standard_normal(n)).astype(np.float32),
    }
    return out


@pytest.mark.parametrize("n", [16, 17, 64, 1000, 4097, 65536])
def test_floor_from_spectrum_equals_the_reference(built_lib, n):
    for name, s in _spectra(n).items():
        for pm in PERMILLES:
            got = capi.floor_from_spectrum(s, floor_permille=pm)
            want = floor_ref.floor_db(s, pm)
            assert floor_ref.same_bits(got, want), (n, name, pm, got, want)
    # the mask's parameters are the descriptor's: no DC mask, another band
    s = _spectra(n)["random"]
    for dc, ub in ((0, 0.75), (2, 0.5), (4, 1.0)):
        got = capi.floor_from_spectrum(s, dc_ignore_bins=dc, use_bandwidth=ub, floor_permille=250)
        assert floor_ref.same_bits(got, floor_ref.floor_db(s, 250, ub, dc)), (n, dc, ub)


def test_the_ranks_are_the_definition_s(built_lib):
    """written out on a spectrum whose evaluated values are known: permille 0 is the median, 1000 the maximum, FLOOR_MIN the
    minimum, and the rank is permille * (M - 1) // 1000 in integers"""
    n = 64
    s = np.arange(n, dtype=np.float32) - 20.0
    from tests import tolerances as tol

    vals = np.sort(s[tol.evaluated_mask(n)])
    M = vals.size
    for pm, r in ((capi.FLOOR_MIN, 0), (1000, M - 1), (0, 500 * (M - 1) // 1000), (500, 500 * (M - 1) // 1000), (1, 0), (999, 999 * (M - 1) // 1000),
                  (250, 250 * (M - 1) // 1000)):
        assert capi.floor_from_spectrum(s, floor_permille=pm) == vals[r], (pm, r)
    # -0.0 ranks below +0.0, bit for bit
    z = np.zeros(n, np.float32)
    z[::2] = -0.0
    assert np.signbit(capi.floor_from_spectrum(z, floor_permille=capi.FLOOR_MIN)) and not np.signbit(capi.floor_from_spectrum(z, floor_permille=1000))


def test_floor_from_spectrum_rejects(built_lib):
    L = capi.lib()
    s = np.zeros(64, np.float32)
    out = C.c_float()
    vp = s.ctypes.data_as(C.c_void_p)
    assert L.scn_floor_from_spectrum(vp, 64, 0, 0.0, 1001, C.byref(out)) == capi.E_INVALID and b"floor_permille" in L.scn_last_error()
    assert L.scn_floor_from_spectrum(None, 64, 0, 0.0, 0, C.byref(out)) == capi.E_INVALID
    assert L.scn_floor_from_spectrum(vp, 64, 0, 0.0, 0, None) == capi.E_INVALID
    assert L.scn_floor_from_spectrum(vp, 0, 0, 0.0, 0, C.byref(out)) == capi.E_INVALID
    assert L.scn_floor_from_spectrum(vp, 64, 4, 0.01, 0, C.byref(out)) == capi.E_INVALID  # the band is the DC mask's bins: nothing is evaluated
    assert L.scn_floor_from_spectrum(vp, 64, 0, 0.0, 0, C.byref(out)) == capi.OK
