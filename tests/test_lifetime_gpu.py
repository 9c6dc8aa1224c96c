"""Everything a plan allocates goes when the plan goes: one plan per route of the C-ABI layer is created, driven through every call
that allocates at first use (submit, collect, scn_collect_more beyond max_hits, signals, the view, the floor, scn_convert_raw,
scn_plan_set_table twice) and destroyed, round after round, and the device's free memory must not fall.

The bound.  The same file was run on the parent commit, whose plans free by hand-written lists (scn_api.hip: free_slot, the tails
of scn_plan_destroy / scn_welch_destroy), with the same R = 20 rounds after one settling round: free memory fell by
0 bytes (PARENT_FALL_BYTES; this tree: 0 bytes as well).  The bound is that plus one 2 MiB allocation granule: the smallest device
allocation a round can forget is a granule, so R forgotten granules are far above it.  (torch.cuda.mem_get_info reads device
memory: a forgotten pinned host buffer or event does not show here.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from scanner_amd import capi

pytestmark = pytest.mark.gpu

ROUNDS = 20
PARENT_FALL_BYTES = 0  # measured: the parent commit's library under this file, ROUNDS = 20 (profiles/api_split.md)
GRANULE = 2 << 20
MAX_HITS = 8
VP = C.c_void_p
KIND_DTYPE = {capi.KIND_FLOAT_COMPLEX: np.float32, capi.KIND_SHORT_COMPLEX: np.int16, capi.KIND_BYTE_COMPLEX: np.int8}
_RNG = np.random.default_rng(7)
_NOISE = _RNG.standard_normal(1 << 20).astype(np.float32)  # drawn once, reused by every plan


def ok(status, where, also=()):
    assert status == capi.OK or status in also, f"{where}: status {status}: {capi.lib().scn_last_error().decode()}"


def raw_samples(kind, count):
    """`count` complex samples of the wire format, as bytes"""
    x = _NOISE[:2 * count]
    if kind == capi.KIND_FLOAT_COMPLEX:
        return x.tobytes()
    return (x * 20.0).astype(KIND_DTYPE[kind]).tobytes()


def drive_plan(L, n, kind=capi.KIND_FLOAT_COMPLEX, slots=(0,), **fields):
    flags = fields.pop("flags", capi.OUT_SPECTRUM | capi.OUT_HITS)
    d = capi.PlanDesc(struct_size=C.sizeof(capi.PlanDesc), n=n, sample_rate=8000000, sample_kind=kind, enob=12, threshold=-300.0,
                      max_batch=4, max_hits=MAX_HITS, flags=flags, **fields)
    plan = VP()
    ok(L.scn_plan_create(C.byref(d), C.byref(plan)), "scn_plan_create")
    nb, units = 4, 4 // max(d.average, 1)
    time_domain = d.mode == capi.MODE_TIME_DOMAIN
    have_hits = bool(flags & capi.OUT_HITS) and not time_domain
    raw = raw_samples(kind, n * nb)
    fc = np.repeat(1e8 + 6e6 * np.arange(units), nb // units)  # (an averaged plan's groups share their centre)
    for slot in slots:
        ptr, size = VP(), C.c_size_t()
        ok(L.scn_host_buffer(plan, slot, C.byref(ptr), C.byref(size)), "scn_host_buffer")
        assert size.value == len(raw)
        C.memmove(ptr, raw, len(raw))
        ok(L.scn_submit(plan, slot, nb, fc.ctypes.data_as(VP), None), "scn_submit")
        if time_domain:
            mx, mn = np.empty(nb, np.float32), np.empty(nb, np.float32)
            ok(L.scn_collect_time_domain(plan, slot, mx.ctypes.data_as(VP), mn.ctypes.data_as(VP), None), "scn_collect_time_domain")
            continue
        power = np.empty((units, n), np.float32) if flags & capi.OUT_SPECTRUM else None
        hits, total = np.empty(MAX_HITS, capi.HIT_DTYPE), C.c_uint32()
        ok(L.scn_collect(plan, slot, power.ctypes.data_as(VP) if power is not None else None, hits.ctypes.data_as(VP) if have_hits else None,
                         MAX_HITS, C.byref(total), None), "scn_collect", also=(capi.E_TRUNCATED,))
        if not have_hits:
            continue
        assert total.value > MAX_HITS + 4, "the threshold lets every evaluated bin through"
        more, wrote = np.empty(total.value, capi.HIT_DTYPE), C.c_uint32()
        ok(L.scn_collect_more(plan, slot, MAX_HITS + 1, more.ctypes.data_as(VP), more.size, C.byref(wrote)), "scn_collect_more")  # beyond max_hits
        assert wrote.value == total.value - MAX_HITS - 1
        sig, n_sig = np.empty(4, capi.SIGNAL_DTYPE), C.c_uint32()
        ok(L.scn_collect_signals(plan, slot, 0, 0, sig.ctypes.data_as(VP), sig.size, C.byref(n_sig)), "scn_collect_signals", also=(capi.E_TRUNCATED,))
        assert n_sig.value >= 1
        view, n_view = VP(), C.c_uint32()
        ok(L.scn_hits_view(plan, slot, C.byref(view), C.byref(n_view)), "scn_hits_view")
        assert n_view.value == MAX_HITS
        if d.detect == capi.DETECT_FLOOR:
            floor = np.empty(units, np.float32)
            ok(L.scn_collect_floor(plan, slot, floor.ctypes.data_as(VP)), "scn_collect_floor")
    converted = np.empty((2, n, 2), np.float32)
    ok(L.scn_convert_raw(plan, raw, 1, converted.ctypes.data_as(VP)), "scn_convert_raw")
    ok(L.scn_convert_raw(plan, raw, 2, converted.ctypes.data_as(VP)), "scn_convert_raw (grown)")
    table = 1e8 + 6e6 * np.arange(8)
    ok(L.scn_plan_set_table(plan, table.ctypes.data_as(VP), 4), "scn_plan_set_table")
    ok(L.scn_plan_set_table(plan, table.ctypes.data_as(VP), 8), "scn_plan_set_table (larger)")
    ok(L.scn_plan_destroy(plan), "scn_plan_destroy")


def drive_welch(L):
    d = capi.WelchDesc(struct_size=C.sizeof(capi.WelchDesc), n=65536, segments_per_psd=2, max_psd=1)
    w, count = VP(), C.c_size_t()
    ok(L.scn_welch_create(C.byref(d), C.byref(w)), "scn_welch_create")
    ok(L.scn_welch_samples(w, 1, C.byref(count)), "scn_welch_samples")
    raw = raw_samples(capi.KIND_FLOAT_COMPLEX, count.value)
    psd = np.empty(65536, np.float32)
    ptr, size = VP(), C.c_size_t()
    ok(L.scn_welch_host_buffer(w, 0, C.byref(ptr), C.byref(size)), "scn_welch_host_buffer")
    C.memmove(ptr, raw, len(raw))
    ok(L.scn_welch_submit(w, 0, 1), "scn_welch_submit")
    ok(L.scn_welch_collect(w, 0, psd.ctypes.data_as(VP)), "scn_welch_collect")
    d_in = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    ok(L.scn_welch_submit_device(w, 1, d_in.data_ptr(), 1, None), "scn_welch_submit_device")
    ok(L.scn_welch_collect(w, 1, psd.ctypes.data_as(VP)), "scn_welch_collect")
    ok(L.scn_welch_destroy(w), "scn_welch_destroy")
    del d_in


def one_round(L):
    drive_plan(L, 16)                                                                              # tiny
    drive_plan(L, 1000)                                                                            # mixed radix
    drive_plan(L, 4096, capi.KIND_SHORT_COMPLEX, slots=(0, 1, 2), flags=capi.OUT_SPECTRUM | capi.OUT_HITS | capi.PLAN_OVERLAP_SLOTS)
    drive_plan(L, 32768, capi.KIND_SHORT_COMPLEX, correct_dc=1)                                    # four-step, both scratch buffers
    drive_plan(L, 17)                                                                              # Bluestein
    drive_plan(L, 1024, average=2)
    drive_plan(L, 64, detect=capi.DETECT_FLOOR, flags=capi.OUT_HITS)
    drive_plan(L, 4096, mode=capi.MODE_TIME_DOMAIN)
    drive_welch(L)
    torch.cuda.synchronize()


def test_rounds_of_plans_leave_the_device_memory_where_it_was(built_lib):
    L = capi.lib()
    one_round(L)  # the runtime settles: its pools, the code objects, torch's context
    torch.cuda.empty_cache()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(ROUNDS):
        one_round(L)
    torch.cuda.empty_cache()
    fall = free_before - torch.cuda.mem_get_info()[0]
    print(f"free device memory fell by {fall} bytes over {ROUNDS} rounds (bound {PARENT_FALL_BYTES + GRANULE})")
    assert fall <= PARENT_FALL_BYTES + GRANULE


def test_a_failed_create_sets_the_error_text(built_lib):
    """scn_plan_create fails in scn_plan.hip, the text is kept by scn_host.hip and read back through scn_last_error: one setter, one
    thread_local, whichever unit reports."""
    L = capi.lib()
    for fields, word in ((dict(n=4096, device_id=1 << 20), b"device_id"), (dict(n=70001), b"unsupported FFT size")):
        d = capi.PlanDesc(struct_size=C.sizeof(capi.PlanDesc), sample_rate=8000000, sample_kind=capi.KIND_FLOAT_COMPLEX, max_batch=4, **fields)
        plan = VP()
        assert L.scn_plan_create(C.byref(d), C.byref(plan)) == capi.E_INVALID and not plan.value
        assert word in L.scn_last_error()
