"""Averaged plans (scn_plan_desc.average / average_layout) on a machine without a GPU: the descriptor's layout and the
checks scn_plan_create makes before it looks for a device."""
import ctypes as C
import os
import subprocess

from scanner_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_desc_layout_and_abi_version(tmp_path):
    assert capi.ABI_VERSION == 6
    assert C.sizeof(capi.PlanDesc) == 88  # the size of ABI version 5: the two fields came out of the reserved words
    f = tmp_path / "t.c"
    f.write_text('#include "scanner_hip.h"\n#include <stddef.h>\nint main(void){ return (int)(sizeof(scn_plan_desc) != %d) + '
                 '(int)(offsetof(scn_plan_desc, average) != %d) + (int)(offsetof(scn_plan_desc, average_layout) != %d) + '
                 '(int)(SCN_ABI_VERSION != 6) + (int)(SCN_AVG_DWELL != %d) + (int)(SCN_AVG_SWEEPS != %d); }\n'
                 % (C.sizeof(capi.PlanDesc), capi.PlanDesc.average.offset, capi.PlanDesc.average_layout.offset,
                    capi.AVG_DWELL, capi.AVG_SWEEPS))
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0, "scn_plan_desc differs between the header and the ctypes binding"


def _desc(**kw):
    d = capi.PlanDesc()
    d.struct_size = C.sizeof(capi.PlanDesc)
    d.n, d.sample_rate, d.sample_kind, d.enob, d.max_batch = 4096, 8000000, capi.KIND_SHORT_COMPLEX, 12, 16
    d.average, d.average_layout = 2, capi.AVG_DWELL
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


def test_invalid_averaged_descriptors(built_lib):
    cases = [
        (dict(average=3, max_batch=4), b"does not divide max_batch"),
        (dict(n=512), b"n = 512 is not supported"),
        (dict(n=16384), b"n = 16384 is not supported"),
        (dict(n=1000), b"n = 1000 is not supported"),
        (dict(mode=capi.MODE_TIME_DOMAIN), b"frequency-domain"),
        (dict(average_layout=2), b"unknown average_layout"),
    ]
    for kw, msg in cases:
        st, err = _create(_desc(**kw))
        assert st == capi.E_INVALID and msg in err and b"average" in err, (kw, st, err)


def test_valid_averaged_descriptors_reach_the_device_check(built_lib):
    """Every valid combination passes the descriptor checks: without a GPU it fails on the device (SCN_E_NO_DEVICE), never
    as SCN_E_INVALID; with one the plan is made."""
    import torch

    want = capi.OK if torch.cuda.is_available() else capi.E_NO_DEVICE
    for n in (1024, 2048, 4096, 8192):
        for layout in (capi.AVG_DWELL, capi.AVG_SWEEPS):
            for avg, mb in ((2, 16), (16, 16), (0, 3), (1, 3), (5, 15)):
                st, err = _create(_desc(n=n, average=avg, average_layout=layout, max_batch=mb))
                assert st == want, (n, layout, avg, mb, st, err)
    # average <= 1 is the plain plan: the averaging checks do not apply (time-domain, other sizes, any layout)
    for kw in (dict(average=1, n=512), dict(average=0, mode=capi.MODE_TIME_DOMAIN, n=7), dict(average=1, average_layout=9)):
        st, err = _create(_desc(**kw))
        assert st == want, (kw, st, err)
